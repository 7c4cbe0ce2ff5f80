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
// GRAD: the same gather, pair loop, factorisation and substitution, then the block's share of the gradient.
// The member at position p is 4s's block on the leading p + 1 rows, so the block's weights are the members' weights summed:
//   W_log = nb sum_p s_p s_p',   W_quad = sum_p [ -N_pp s_p s_p' - (h_p s_p' + s_p h_p') ],   N = sum_c w_c w_c',
// with s_p = L^-T e_p (row p of L^-1) and h_p = L_{0..p}^-T N[p, 0..p).  The substitution leaves N's member rows in LDS, the
// members' backward solves are dealt over the four wavefronts, and every pair's partials are evaluated ONCE by one of the
// VECCHIA_GROUP_THREADS threads and weighted with the two sums over the members, ascending.  One record per block.
//
//
// FISH: the same gather, pair loop and factorisation, the members' backward solves without h, then the block's
// share of the expected information.  The member at position p is 4t's block on the leading p + 1 rows: with
// q_{a,p} = C_a[0..p, 0..p] s_p and g_{a,p} = L_{0..p}^-1 q_{a,p} it gives sum_{j < p} g_a[j] g_b[j] + g_a[p] g_b[p] / 2, and the
// block the sum over its members.  The factor stays in LDS for the forward solves; every pair's partials are evaluated once
// per walk and serve all the members of a chunk and all the directions of a group.  One record per block.
//
// COEF: the same gather, pair loop and factorisation, then the members' backward solves s_p = L_{0..p}^-T e_p
// as vecchia_coef_kernel runs them on the leading (p + 1) x (p + 1) sub-block -- component j is
// (e_p[j] - sum_{i > j} L(i, j) s_p[i]) / L(j, j), i descending from p, DIVIDED by the pivot -- and every s_p goes straight
// into its row's record of launch_vecchia_coefs.  The factor's bits are the ungrouped leading sub-block's (above), the solve
// reads nothing else, so the records are the bits of the ungrouped launch on the same table.  The members are dealt over
// the four wavefronts by rank, and a wavefront solves VECCHIA_G of its members at a time: they share the read of the
// factor's row and give the shuffles four independent chains.
//
// Compile with -ffp-contract=off, like vecchia.hip: the products and sums stand as written.
#include <hip/hip_runtime.h>
#include <atomic>
#include "kernels.h"
#include "matern_device.hpp"
#include "grad_pair.hpp"
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
// GRAD (vecchia_group_grad_lds_bytes) keeps tri at VECCHIA_GROUP_STG doubles or more -- once the members' solves are done the
// factor is dead and the pair walk stages a pass of VECCHIA_GROUP_THREADS pairs there -- and puts behind it:
//   sm    kb (kb + 1) / 2    row p of a member: s_p;
//   nm    kb (kb + 1) / 2    row p of a member: N[p, 0..p], then h_p in the places 0 .. p - 1 (the diagonal keeps N_pp);
//   sp    GSITE_FIELDS x kb  the rows' site derivatives as an SoA of stride kb;
//   ys, uv  kb each          sum_c y_pc of the members, and u = sum_p ys[p] s_p;
//   gs    2 GFAM x kb        the rows' site sums: the log-determinant's share per family, then the quadratic forms';
//   red   2 x 4              the wavefronts' shares of the two global-range sums.
// FISH (vecchia_group_fisher_lds_bytes) keeps the factor in tri and puts behind it, for chunks of mc members and groups of gd
// directions (vecchia_group_fisher_shape):
//   sm    kb (kb + 1) / 2    row p of a member: s_p;
//   sp    VECCHIA_FX x kb    the rows' site derivatives, then the members' positions, ascending (kb ints);
//   wts   gd x GFAM x kb     the rows' site weights w_a[f][row] of the group's directions;
//   stg   gd x T             a pass of T = VECCHIA_GROUP_THREADS pairs: the entry of C_a per direction (and, once per chunk,
//                            the members' sums u_p of the mean block: mc x p <= 4 T doubles);
//   gall  mc x ndir x kb     g_{a,p} of the chunk's members and every direction, what the Gram is formed of.
constexpr int VECCHIA_GROUP_STGF = 2 * GFAM + 2;        // a staged pair: da, db, 2 W_log, 2 W_quad
constexpr int VECCHIA_GROUP_STG = VECCHIA_GROUP_STGF * VECCHIA_GROUP_THREADS;
constexpr int VECCHIA_GROUP_GX = GSITE_FIELDS + 2 + 2 * GFAM;
constexpr int VECCHIA_GROUP_WAVES = VECCHIA_GROUP_THREADS / 64;
static_assert(2 * GFAM % VECCHIA_GROUP_WAVES == 0, "the site sums are dealt evenly over the wavefronts");

__device__ __forceinline__ double vecchia_group_wave_sum(double v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int VECCHIA_GROUP_FQ = 16;                   // FISH: (member, direction) accumulators a thread keeps
static_assert(VECCHIA_GROUP_FQ == VECCHIA_FD && VECCHIA_GROUP_FQ % VECCHIA_G == 0, "a thread's accumulators go through "
              "vecchia_forward four at a time, and one wavefront can hold a whole group of directions of one member");
static_assert(COCONS_P_MAX * (VECCHIA_GROUP_FQ * VECCHIA_GROUP_WAVES / VECCHIA_G) <= VECCHIA_G * VECCHIA_GROUP_THREADS,
              "the members' sums u_p of a chunk fit the staging of the narrowest group");

template <int MODE, bool GRAD = false, bool FISH = false, bool COEF = false>
__global__ void __launch_bounds__(VECCHIA_GROUP_THREADS)
vecchia_group_kernel(VecchiaGroupArgs a)
{
    static_assert(!(GRAD && FISH) && !(COEF && (GRAD || FISH)), "the gradient, the information and the coefficients are "
                  "launches of their own");
    constexpr bool DER = GRAD || FISH;             // the launches that gather the site derivatives and solve for the s_p
    extern __shared__ double vecchia_group_lds[];
    const int lane = threadIdx.x, kb = a.kb;
    const int blk = (DER ? a.blk0 : 0) + (a.order ? a.order[blockIdx.x] : (int)blockIdx.x);
    const int off = a.off[blk], nrows = a.off[blk + 1] - off;
    const unsigned long long members = a.mask[blk];
    const int ntri = kb * (kb + 1) / 2;
    double *par = vecchia_group_lds;
    double *tri = par + LOCP_FIELDS * kb;
    [[maybe_unused]] double *sm = tri + ((GRAD && ntri < VECCHIA_GROUP_STG) ? VECCHIA_GROUP_STG : ntri);
    [[maybe_unused]] double *nm = sm + ntri;
    [[maybe_unused]] double *sp = FISH ? nm : nm + ntri;          // (FISH has no rows of N)
    int *nb = GRAD   ? (int *)(sp + VECCHIA_GROUP_GX * kb + 2 * VECCHIA_GROUP_WAVES)
              : FISH ? (int *)(sp + VECCHIA_FX * kb + a.gd * (GFAM * kb + VECCHIA_GROUP_THREADS) + a.ndir * a.mc * kb)
                     : (int *)(tri + ntri);
    if (nrows < 1 || nrows > kb) return;          // (a plan the host checked has none)
    // COEF: the rows below row0 are fixed.  The rows ascend, so a block whose last row is fixed has nothing to give
    if (COEF && a.rows[off + nrows - 1] < a.row0) return;

    if (lane < nrows) nb[lane] = a.rows[off + lane];
    __syncthreads();
    for (int e = lane; e < nrows * VECCHIA_REC; e += VECCHIA_GROUP_THREADS) {
        const int r = e / VECCHIA_REC, f = e % VECCHIA_REC;
        if (f >= LOCP_FIELDS) continue;
        par[f * kb + r] = a.aosK[(size_t)nb[r] * VECCHIA_REC + f];
    }
    if constexpr (DER) {
        for (int e = lane; e < nrows * VECCHIA_GSITE_REC; e += VECCHIA_GROUP_THREADS) {
            const int r = e / VECCHIA_GSITE_REC, f = e % VECCHIA_GSITE_REC;
            sp[f * kb + r] = a.aosG[(size_t)nb[r] * VECCHIA_GSITE_REC + f];
        }
        if constexpr (GRAD)
            for (int e = lane; e < nrows * (nrows + 1) / 2; e += VECCHIA_GROUP_THREADS) nm[e] = 0.0;
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
        // the members from position `bad` on fail; the last row of a block is a member, so there is one (COEF: and its row
        // is not fixed, so the first member from `bad` on that is not fixed exists too)
        unsigned long long late = members >> bad;
        if constexpr (COEF)
            while (late && nb[bad + __builtin_ctzll(late)] < a.row0) late &= late - 1;
        const int q = late ? bad + __builtin_ctzll(late) : nrows;
        if (lane == 0 && q < nrows) atomicMin(a.fail, nb[q] + 1);
        return;
    }
    if ((DER || COEF) && lane < nrows) tri[tri_at(lane, lane)] = piv_mine;   // (the solves of the other wavefronts read the pivots here)
    __syncthreads();
    if constexpr (COEF) {
        // No barrier from here on: a wavefront that carries no member's solve falls through the loop and ends.
        // Member i (ascending, among those whose row is not fixed) is wavefront i mod 4's, lane = row; a wavefront takes
        // VECCHIA_G of its members at a time.  Step j is one column of L' (a row of the packed factor): the lanes read it once
        // for the members of the batch, a member at a position below j sits the step out.
        const int wv = lane >> 6, ln = lane & 63;
        const double pivl = ln < nrows ? tri[tri_at(ln, ln)] : 1.0;
        const int nfix = __popcll(__ballot(ln < nrows && nb[ln] < a.row0));      // (rows ascending: the fixed ones lead)
        unsigned long long rest = members & (~0ull << nfix);                     // (nfix <= nrows - 1 <= 63)
        for (int rank = 0; rest;) {
            int pg[VECCHIA_G], cnt = 0;
            for (; rest && cnt < VECCHIA_G; rest &= rest - 1, ++rank)
                if ((rank & (VECCHIA_GROUP_WAVES - 1)) == wv) pg[cnt++] = __builtin_ctzll(rest);
            if (!cnt) break;
            for (int g = cnt; g < VECCHIA_G; ++g) pg[g] = -1;
            double rs[VECCHIA_G], sv[VECCHIA_G];
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) { rs[g] = ln == pg[g] ? 1.0 : 0.0; sv[g] = 0.0; }
            for (int j = pg[cnt - 1]; j >= 0; --j) {
                const double l = ln < j ? tri[tri_at(j, 0) + ln] : 0.0;
#pragma unroll
                for (int g = 0; g < VECCHIA_G; ++g) {
                    if (j > pg[g]) continue;                                     // (the same in every lane)
                    const double xs = __shfl(rs[g] / pivl, j);
                    if (ln == j) sv[g] = xs;
                    if (ln < j) rs[g] -= l * xs;
                }
            }
            const int m = (int)a.ldc - 1;
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) {
                if (pg[g] < 0) continue;
                double *rec = a.coef + (size_t)nb[pg[g]] * a.ldc;
                if (ln < m) rec[ln] = ln < pg[g] ? sv[g] : 0.0;
                if (ln == pg[g]) rec[m] = sv[g];
            }
        }
        return;
    }
    if (!DER && lane >= 64) return;                // (no barrier from here on)
    // forward substitution, VECCHIA_G right-hand sides at a time: lane r ends with b_r - sum_{j < r} C(r, j) y_j, j ascending.
    // A lane at or in front of step j takes no part in it: its value must not see a y_j that is not finite.
    // GRAD: every lane j ends with the numerator of w_c[j], so N[p, j] = sum_c w_c[p] w_c[j] of the member rows p >= j and
    // sum_c w_c[p] are formed on the way, the columns ascending.
    const bool member = lane < nrows && ((members >> lane) & 1ull);
    const int site = lane < nrows ? nb[lane] : 0;
    [[maybe_unused]] double ysum = 0.0;
    for (int c0 = 0; !FISH && lane < 64 && c0 < a.nb; c0 += VECCHIA_G) {   // (GRAD: the other wavefronts go on to the barrier)
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
        if constexpr (GRAD) {
            double w[VECCHIA_G];
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) w[g] = (lane < nrows && c0 + g < a.nb) ? b[g] / piv_mine : 0.0;
            for (unsigned long long rest = members; rest; rest &= rest - 1) {
                const int p = __builtin_ctzll(rest);
                double acc = lane <= p ? nm[tri_at(p, lane)] : 0.0;
#pragma unroll
                for (int g = 0; g < VECCHIA_G; ++g) {
                    if (c0 + g >= a.nb) break;
                    const double y = __shfl(w[g], p);
                    acc += y * w[g];
                }
                if (lane <= p) nm[tri_at(p, lane)] = acc;
            }
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) {
                if (c0 + g >= a.nb) break;
                ysum += w[g];
            }
        }
    }
    if (!FISH && member && a.logd) a.logd[site] = log(piv_mine);
    if constexpr (GRAD) {
        const int wv = lane >> 6, ln = lane & 63, T = VECCHIA_GROUP_THREADS;
        double *ys = sp + GSITE_FIELDS * kb, *uv = ys + kb, *gs = uv + kb, *red = gs + 2 * GFAM * kb;
        if (lane < nrows) ys[lane] = ysum;
        __syncthreads();
        // The members' backward solves, member i (ascending) on wavefront i mod 4, lane = row: one column of L' (a row of the
        // packed factor) per step, s_p and h_p together as in 4s.  h_p takes the place of N[p, 0..p) -- the wavefront that
        // owns the member is the only one that touches its row.
        {
            const double ipiv = ln < nrows ? 1.0 / tri[tri_at(ln, ln)] : 0.0;
            int rank = 0;
            for (unsigned long long rest = members; rest; rest &= rest - 1, ++rank) {
                if ((rank & (VECCHIA_GROUP_WAVES - 1)) != wv) continue;
                const int p = __builtin_ctzll(rest);
                double rs = ln == p ? 1.0 : 0.0, rh = ln < p ? nm[tri_at(p, ln)] : 0.0, s_mine = 0.0, h_mine = 0.0;
                for (int j = p; j >= 0; --j) {
                    const double xs = __shfl(rs * ipiv, j), xh = __shfl(rh * ipiv, j);
                    if (ln == j) { s_mine = xs; h_mine = xh; }
                    if (ln < j) {
                        const double l = tri[tri_at(j, 0) + ln];
                        rs -= l * xs;
                        rh -= l * xh;
                    }
                }
                if (ln <= p) sm[tri_at(p, ln)] = s_mine;
                if (ln < p) nm[tri_at(p, ln)] = h_mine;
            }
        }
        __syncthreads();                   // the factor is dead from here on, tri is the staging of the pair walk
        // The weights of the pair (r, c), r >= c: the members at the positions p >= r, ascending
        const double cn = (double)a.nb;
        auto weights = [&](int r, int c, double &wl, double &wq) {
            double sl = 0.0, sq = 0.0;
            for (unsigned long long rest = members & (~0ull << r); rest; rest &= rest - 1) {
                const int p = __builtin_ctzll(rest), at = tri_at(p, 0);
                const double zr = sm[at + r], zc = sm[at + c], npp = nm[at + p];
                const double hr = r < p ? nm[at + r] : 0.0, hc = c < p ? nm[at + c] : 0.0;
                sl += zr * zc;
                sq += 0.0 - npp * (zr * zc) - (hr * zc + zr * hc);
            }
            wl = cn * sl;
            wq = sq;
        };
        // thread (row ln, wavefront wv) keeps VECCHIA_GROUP_NACC of the row's 2 GFAM site sums, q = wv NACC + i: the
        // log-determinant's share of family q below GFAM, the quadratic forms' of family q - GFAM from there on
        constexpr int NACC = 2 * GFAM / VECCHIA_GROUP_WAVES;
        const int q0 = wv * NACC, f0 = q0 % GFAM, wsel = 2 * GFAM + (q0 >= GFAM ? 1 : 0);
        double acc[NACC];
#pragma unroll
        for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
        if (ln < nrows) {
            // the diagonal first: W_aa (exp(eta_sd), nugget)
            double wl, wq;
            weights(ln, ln, wl, wq);
            const double w = q0 >= GFAM ? wq : wl, dsd = sp[3 * kb + ln], dng = par[12 * kb + ln];
#pragma unroll
            for (int i = 0; i < NACC; ++i) {
                if (f0 + i == TH_SD_) acc[i] = w * dsd;
                if (f0 + i == TH_NG_) acc[i] = w * dng;
            }
            if (wv == 0) {
                // u = sum_p (sum_c y_pc) s_p over the members at the positions p >= ln, ascending
                double u = 0.0;
                for (unsigned long long rest = members & (~0ull << ln); rest; rest &= rest - 1) {
                    const int p = __builtin_ctzll(rest);
                    u += ys[p] * sm[tri_at(p, ln)];
                }
                uv[ln] = u;
            }
        }
        // The pair walk: VECCHIA_GROUP_THREADS pairs a pass, one per thread (the order of the assembly above), each pair's
        // partials evaluated once and staged with 2 W_log and 2 W_quad; then thread (a, wv) adds what the pass holds for its
        // site -- its pairs (a, c), c < a ascending (the jj side), then its pairs (r, a), r > a ascending (the ii side).
        double *stg = tri;
        double glob_l = 0.0, glob_q = 0.0;
        for (int t0 = 0; t0 < npairs; t0 += T) {
            const int t = t0 + lane;
            double da[GFAM], db[GFAM], dg = 0.0, w2l = 0.0, w2q = 0.0;
#pragma unroll
            for (int f = 0; f < GFAM; ++f) { da[f] = 0.0; db[f] = 0.0; }
            if (t < npairs) {
                int r, c;
                tri_pair(t, r, c);
                pair_partials<MODE>(par, (size_t)kb, sp, (size_t)kb, a.gr, a.nu_fixed, a.smooth_free, c, r, da, db, dg);
                double wl, wq;
                weights(r, c, wl, wq);
                w2l = 2.0 * wl;
                w2q = 2.0 * wq;
                glob_l += w2l * dg;
                glob_q += w2q * dg;
            }
#pragma unroll
            for (int f = 0; f < GFAM; ++f) {
                stg[f * T + lane] = da[f];
                stg[(GFAM + f) * T + lane] = db[f];
            }
            stg[2 * GFAM * T + lane] = w2l;
            stg[(2 * GFAM + 1) * T + lane] = w2q;
            __syncthreads();
            if (ln < nrows) {
                const int tend = min(t0 + T, npairs), mine0 = ln * (ln - 1) / 2;
                for (int u = max(t0, mine0); u < min(tend, mine0 + ln); ++u) {
                    const double w = stg[wsel * T + (u - t0)];
#pragma unroll
                    for (int i = 0; i < NACC; ++i) acc[i] += w * stg[(GFAM + f0 + i) * T + (u - t0)];
                }
                int r_lo, r_hi, c_;
                tri_pair(t0, r_lo, c_);
                tri_pair(tend - 1, r_hi, c_);
                for (int r = max(r_lo, ln + 1); r <= r_hi; ++r) {
                    const int u = r * (r - 1) / 2 + ln;
                    if (u < t0 || u >= tend) continue;
                    const double w = stg[wsel * T + (u - t0)];
#pragma unroll
                    for (int i = 0; i < NACC; ++i) acc[i] += w * stg[(f0 + i) * T + (u - t0)];
                }
            }
            __syncthreads();
        }
        if (ln < nrows) {
#pragma unroll
            for (int i = 0; i < NACC; ++i) gs[(q0 + i) * kb + ln] = acc[i];
        }
        // the global-range sums: a fixed butterfly per wavefront, the wavefronts' shares added in their order
        glob_l = vecchia_group_wave_sum(glob_l);
        glob_q = vecchia_group_wave_sum(glob_q);
        if (ln == 0) { red[wv] = glob_l; red[VECCHIA_GROUP_WAVES + wv] = glob_q; }
        __syncthreads();
        // the record, at the block's id: the site sums contracted with X over the block's rows, ascending
        const int p = a.p, b = blk - a.blk0;
        for (int o = lane; o < (2 * GFAM + 1) * p; o += T) {
            const int q = o / p, kx = o % p;
            const double *g = q < 2 * GFAM ? gs + q * kb : uv;
            double s = 0.0;
            for (int rr = 0; rr < nrows; ++rr) s += g[rr] * a.X[(size_t)nb[rr] + (size_t)kx * a.ldx];
            if (q < 2 * GFAM) a.rec[(size_t)o * a.ldr + b] = s;
            else a.rec[(size_t)(2 * GFAM * p + 2 + kx) * a.ldr + b] = s;
        }
        if (lane == 0) {
            double gl = red[0], gq = red[VECCHIA_GROUP_WAVES];
            for (int w = 1; w < VECCHIA_GROUP_WAVES; ++w) { gl += red[w]; gq += red[VECCHIA_GROUP_WAVES + w]; }
            a.rec[(size_t)(2 * GFAM * p) * a.ldr + b] = gl;
            a.rec[(size_t)(2 * GFAM * p + 1) * a.ldr + b] = gq;
        }
    }
    if constexpr (FISH) {
        const int wv = lane >> 6, ln = lane & 63, T = VECCHIA_GROUP_THREADS;
        const int p = a.p, ndir = a.ndir, gw = a.gd, mc = a.mc, b = blk - a.blk0;
        const int ng = ndir * (ndir + 1) / 2, nmem = __popcll(members);
        int *mpos = (int *)(sp + GSITE_FIELDS * kb);
        double *wts = sp + VECCHIA_FX * kb, *stg = wts + gw * GFAM * kb, *gall = stg + gw * T;
        if (member) mpos[__popcll(members & ((1ull << lane) - 1ull))] = lane;
        // The members' backward solves as in GRAD, without h: member i (ascending) on wavefront i mod 4, lane = row.
        {
            const double ipiv = ln < nrows ? 1.0 / tri[tri_at(ln, ln)] : 0.0;
            int rank = 0;
            for (unsigned long long rest = members; rest; rest &= rest - 1, ++rank) {
                if ((rank & (VECCHIA_GROUP_WAVES - 1)) != wv) continue;
                const int pp = __builtin_ctzll(rest);
                double rs = ln == pp ? 1.0 : 0.0, s_mine = 0.0;
                for (int j = pp; j >= 0; --j) {
                    const double xs = __shfl(rs * ipiv, j);
                    if (ln == j) s_mine = xs;
                    if (ln < j) rs -= tri[tri_at(j, 0) + ln] * xs;
                }
                if (ln <= pp) sm[tri_at(pp, ln)] = s_mine;
            }
        }
        __syncthreads();
        // every wavefront solves forward with lane = row: its row of the factor and its pivot
        const int wrow = tri_at(ln, 0);
        const double wpiv = ln < nrows ? tri[tri_at(ln, ln)] : 1.0;
        // A thread's VECCHIA_GROUP_FQ accumulators are the slots x = wv FQ + i of the chunk: member x / gw of the chunk,
        // direction x mod gw of the group.  gw is a multiple of VECCHIA_G, so four slots in a row share their member.
        constexpr int NQ = VECCHIA_GROUP_FQ, NB = NQ / VECCHIA_G;
        for (int m0 = 0; m0 < nmem; m0 += mc) {
            const int cm = min(mc, nmem - m0);
            // u_p = sum_{row <= p} s_p[row] X[site(row), .] of the chunk's members, the rows ascending, and their share of the
            // mean block: entry (k, l) is one thread's running sum over all the members, ascending, kept in the record
            for (int e = lane; e < cm * p; e += T) {
                const int pp = mpos[m0 + e / p], kx = e % p;
                const double *sv = sm + tri_at(pp, 0);
                double s = 0.0;
                for (int rr = 0; rr <= pp; ++rr) s += sv[rr] * a.X[(size_t)nb[rr] + (size_t)kx * a.ldx];
                stg[e] = s;
            }
            __syncthreads();
            for (int o = lane; o < p * (p + 1) / 2; o += T) {
                int ra, cb;
                tri_pair(o, ra, cb);
                double *dst = a.rec + (size_t)(ng + o) * a.ldr + b;
                double s = m0 ? *dst : 0.0;
                for (int mi = 0; mi < cm; ++mi) s += stg[mi * p + ra - 1] * stg[mi * p + cb];
                *dst = s;
            }
            int pm[NB], db[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int x = wv * NQ + k * VECCHIA_G, mi = x / gw;
                pm[k] = mi < cm ? mpos[m0 + mi] : -1;
                db[k] = x % gw;
            }
            for (int d0 = 0; d0 < ndir; d0 += gw) {
                const int gd = min(gw, ndir - d0);
                __syncthreads();           // the sums u_p, or the previous group's walk, have left wts and stg
                // the site weights of the group's directions (vecchia_block_kernel's, 4t step 1)
                for (int e = lane; e < gd * GFAM * nrows; e += T) {
                    const int rr = e % nrows, f = (e / nrows) % GFAM, d = e / (nrows * GFAM);
                    const double *v = a.dirs + ((size_t)(d0 + d) * GFAM + f) * p;
                    double w = 0.0;
                    for (int kx = (f == TH_SCALE_ ? 1 : 0); kx < p; ++kx) w += a.X[(size_t)nb[rr] + (size_t)kx * a.ldx] * v[kx];
                    wts[(d * GFAM + f) * kb + rr] = f == TH_SCALE_ ? 2.0 * w : w;
                }
                __syncthreads();
                // q_{a,p}[row] in registers: the diagonal first, then the row's pairs pass by pass (the gradient walk's order)
                double q[NQ];
#pragma unroll
                for (int i = 0; i < NQ; ++i) q[i] = 0.0;
                if (ln < nrows) {
                    const double dsd = sp[3 * kb + ln], dng = par[12 * kb + ln];
#pragma unroll
                    for (int k = 0; k < NB; ++k) {
                        if (pm[k] < ln) continue;
                        const double so = sm[tri_at(pm[k], ln)];
#pragma unroll
                        for (int g = 0; g < VECCHIA_G; ++g) {
                            const int d = db[k] + g;
                            if (d < gd)
                                q[k * VECCHIA_G + g] =
                                    (dsd * wts[(d * GFAM + TH_SD_) * kb + ln] + dng * wts[(d * GFAM + TH_NG_) * kb + ln]) * so;
                        }
                    }
                }
                for (int t0 = 0; t0 < npairs; t0 += T) {
                    const int t = t0 + lane;
                    double da[GFAM], db_[GFAM], dg = 0.0;
                    int r = 0, c = 0;
#pragma unroll
                    for (int f = 0; f < GFAM; ++f) { da[f] = 0.0; db_[f] = 0.0; }
                    if (t < npairs) {
                        tri_pair(t, r, c);
                        pair_partials<MODE>(par, (size_t)kb, sp, (size_t)kb, a.gr, a.nu_fixed, a.smooth_free, c, r, da, db_, dg);
                    }
                    for (int d = 0; d < gd; ++d) {
                        double e = 0.0;
                        if (t < npairs) {
                            const double *w = wts + d * GFAM * kb;
                            e = dg * a.dirs[((size_t)(d0 + d) * GFAM + TH_SCALE_) * p];
#pragma unroll
                            for (int f = 0; f < GFAM; ++f) {
                                e += da[f] * w[f * kb + c];
                                e += db_[f] * w[f * kb + r];
                            }
                        }
                        stg[d * T + lane] = e;
                    }
                    __syncthreads();
                    if (ln < nrows) {
                        // the row's pairs (ln, c), c ascending, then (r, ln), r ascending; member p takes the pairs with r <= p
                        const int tend = min(t0 + T, npairs), mine0 = ln * (ln - 1) / 2;
                        for (int u = max(t0, mine0); u < min(tend, mine0 + ln); ++u) {
#pragma unroll
                            for (int k = 0; k < NB; ++k) {
                                if (pm[k] < ln) continue;
                                const double so = sm[tri_at(pm[k], 0) + (u - mine0)];
#pragma unroll
                                for (int g = 0; g < VECCHIA_G; ++g)
                                    if (db[k] + g < gd) q[k * VECCHIA_G + g] += stg[(db[k] + g) * T + (u - t0)] * so;
                            }
                        }
                        int r_lo, r_hi, c_;
                        tri_pair(t0, r_lo, c_);
                        tri_pair(tend - 1, r_hi, c_);
                        for (int rr = max(r_lo, ln + 1); rr <= r_hi; ++rr) {
                            const int u = rr * (rr - 1) / 2 + ln;
                            if (u < t0 || u >= tend) continue;
#pragma unroll
                            for (int k = 0; k < NB; ++k) {
                                if (pm[k] < rr) continue;
                                const double so = sm[tri_at(pm[k], 0) + rr];
#pragma unroll
                                for (int g = 0; g < VECCHIA_G; ++g)
                                    if (db[k] + g < gd) q[k * VECCHIA_G + g] += stg[(db[k] + g) * T + (u - t0)] * so;
                            }
                        }
                    }
                    __syncthreads();
                }
                // g_{a,p} = L_{0..p}^-1 q_{a,p}: the likelihood's substitution on the leading p + 1 rows (pm and db are the
                // same in every lane of a wavefront)
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    if (pm[k] < 0 || db[k] >= gd) continue;
                    double bb[VECCHIA_G];
#pragma unroll
                    for (int g = 0; g < VECCHIA_G; ++g) bb[g] = q[k * VECCHIA_G + g];
                    vecchia_forward(bb, tri, wrow, wpiv, ln, pm[k], pm[k] + 1);
                    const int mi = (wv * NQ + k * VECCHIA_G) / gw;
#pragma unroll
                    for (int g = 0; g < VECCHIA_G; ++g)
                        if (db[k] + g < gd && ln <= pm[k]) gall[((size_t)mi * ndir + d0 + db[k] + g) * kb + ln] = bb[g] / wpiv;
                }
            }
            __syncthreads();
            // The chunk's share of the Gram, entry o = a (a + 1) / 2 + b: one thread's running sum over all the members,
            // ascending, the rows ascending within a member -- kept in the record from chunk to chunk, so it does not depend on
            // mc
            for (int o = lane; o < ng; o += T) {
                int ra, cb;
                tri_pair(o, ra, cb);       // (the strict triangle's numbering of (a + 1, b))
                double *dst = a.rec + (size_t)o * a.ldr + b;
                double s = m0 ? *dst : 0.0;
                for (int mi = 0; mi < cm; ++mi) {
                    const int pp = mpos[m0 + mi];
                    const double *ga = gall + ((size_t)mi * ndir + ra - 1) * kb, *gb = gall + ((size_t)mi * ndir + cb) * kb;
                    for (int j = 0; j < pp; ++j) s += ga[j] * gb[j];
                    s += 0.5 * (ga[pp] * gb[pp]);
                }
                *dst = s;
            }
            __syncthreads();               // (the next chunk writes stg and gall)
        }
    }
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

void launch_vecchia_group_coefs(int mode, const VecchiaGroupArgs &a, hipStream_t s)
{
    if (a.blocks <= 0) return;
    const size_t shm = vecchia_lds_bytes(a.kb - 1, false);    // the value launch's layout: the s_p go straight to memory
    const dim3 grid((unsigned)a.blocks), block(VECCHIA_GROUP_THREADS);
    switch (mode) {
    case MODE_HALF: hipLaunchKernelGGL((vecchia_group_kernel<MODE_HALF, false, false, true>), grid, block, shm, s, a); break;
    case MODE_THREEHALF: hipLaunchKernelGGL((vecchia_group_kernel<MODE_THREEHALF, false, false, true>), grid, block, shm, s, a); break;
    case MODE_FIVEHALF: hipLaunchKernelGGL((vecchia_group_kernel<MODE_FIVEHALF, false, false, true>), grid, block, shm, s, a); break;
    default: hipLaunchKernelGGL((vecchia_group_kernel<MODE_GEOM, false, false, true>), grid, block, shm, s, a); break;
    }
}

size_t vecchia_group_grad_lds_bytes(int kb)
{
    const size_t k = (size_t)kb, ntri = k * (k + 1) / 2;
    return (LOCP_FIELDS * k + (ntri < (size_t)VECCHIA_GROUP_STG ? (size_t)VECCHIA_GROUP_STG : ntri) + 2 * ntri +
            VECCHIA_GROUP_GX * k + 2 * VECCHIA_GROUP_WAVES) * sizeof(double) + k * sizeof(int);
}

template <int MODE> static void vecchia_group_grad_launch(const VecchiaGroupArgs &a, size_t shm, hipStream_t s)
{
    static std::atomic<unsigned long long> attr_done{0};
    if (shm > 64 * 1024)
        set_dynamic_lds_once((const void *)vecchia_group_kernel<MODE, true>, vecchia_group_grad_lds_bytes(64), attr_done);
    hipLaunchKernelGGL((vecchia_group_kernel<MODE, true>), dim3((unsigned)a.blocks), dim3(VECCHIA_GROUP_THREADS), shm, s, a);
}

void launch_vecchia_group_grad_blocks(int mode, const VecchiaGroupArgs &a, hipStream_t s)
{
    if (a.blocks <= 0) return;
    const size_t shm = vecchia_group_grad_lds_bytes(a.kb);    // kb <= 64: at most 78 144 bytes
    switch (mode) {
    case MODE_HALF: vecchia_group_grad_launch<MODE_HALF>(a, shm, s); break;
    case MODE_THREEHALF: vecchia_group_grad_launch<MODE_THREEHALF>(a, shm, s); break;
    case MODE_FIVEHALF: vecchia_group_grad_launch<MODE_FIVEHALF>(a, shm, s); break;
    default: vecchia_group_grad_launch<MODE_GEOM>(a, shm, s); break;
    }
}

// FISH.  The shape of a launch: a thread keeps VECCHIA_GROUP_FQ = 16 accumulators and the four wavefronts 64 slots, so gd
// directions a group leave 64 / gd members a chunk.  gd is the smallest of 4, 8, 16 that holds ndir (16 from ndir = 9 on: the
// fewest pair walks, ceil(members / mc) ceil(ndir / gd)), mc = 64 / gd; while the LDS is above VECCHIA_FISHER_LDS_MAX first mc
// is halved (gall shrinks), then gd (wts and stg shrink).
size_t vecchia_group_fisher_lds_bytes(int kb, int ndir, int gd, int mc)
{
    const size_t k = (size_t)kb, ntri = k * (k + 1) / 2;
    return (LOCP_FIELDS * k + 2 * ntri + VECCHIA_FX * k + (size_t)gd * (GFAM * k + VECCHIA_GROUP_THREADS) +
            (size_t)ndir * mc * k) * sizeof(double) + k * sizeof(int);
}

void vecchia_group_fisher_shape(int kb, int ndir, int *gd_out, int *mc_out)
{
    int gd = VECCHIA_G;
    while (gd < VECCHIA_GROUP_FQ && gd < ndir) gd *= 2;
    int mc = VECCHIA_GROUP_FQ * VECCHIA_GROUP_WAVES / gd;
    while (mc > 1 && vecchia_group_fisher_lds_bytes(kb, ndir, gd, mc) > VECCHIA_FISHER_LDS_MAX) mc /= 2;
    while (gd > VECCHIA_G && vecchia_group_fisher_lds_bytes(kb, ndir, gd, mc) > VECCHIA_FISHER_LDS_MAX) gd /= 2;
    *gd_out = gd;
    *mc_out = mc;
}

template <int MODE> static void vecchia_group_fisher_launch(const VecchiaGroupArgs &a, size_t shm, hipStream_t s)
{
    static std::atomic<unsigned long long> attr_done{0};
    if (shm > 64 * 1024)
        set_dynamic_lds_once((const void *)vecchia_group_kernel<MODE, false, true>, VECCHIA_FISHER_LDS_MAX, attr_done);
    hipLaunchKernelGGL((vecchia_group_kernel<MODE, false, true>), dim3((unsigned)a.blocks), dim3(VECCHIA_GROUP_THREADS), shm, s,
                       a);
}

void launch_vecchia_group_fisher_blocks(int mode, const VecchiaGroupArgs &a, hipStream_t s)
{
    if (a.blocks <= 0) return;
    const size_t shm = vecchia_group_fisher_lds_bytes(a.kb, a.ndir, a.gd, a.mc);
    switch (mode) {
    case MODE_HALF: vecchia_group_fisher_launch<MODE_HALF>(a, shm, s); break;
    case MODE_THREEHALF: vecchia_group_fisher_launch<MODE_THREEHALF>(a, shm, s); break;
    case MODE_FIVEHALF: vecchia_group_fisher_launch<MODE_FIVEHALF>(a, shm, s); break;
    default: vecchia_group_fisher_launch<MODE_GEOM>(a, shm, s); break;
    }
}

}  // namespace cocons
