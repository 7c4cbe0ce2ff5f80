// vecchia_group.hip -- grouped Vecchia blocks (gfx950): one workgroup per block of up to 64 rows.  Its first
// wavefront factors and solves with lane = row; all VECCHIA_GROUP_THREADS threads gather the records and evaluate the pairs.
//
// A block holds the rows S = (its members and all their neighbours), ascending.  The member at position p conditions on the
// positions 0 .. p - 1, so its term is what the ungrouped kernels of vecchia.hip compute on the leading (p + 1) x (p + 1)
// sub-block -- through the SAME phases (vecchia_block.hpp):
//   - vecchia_assemble evaluates the same pairs with the earlier row on the `ii` side;
//   - vecchia_factor touches element (r, c) in ascending j only, with operands of the leading sub-block;
//   - the forward substitution subtracts in ascending j only, and the steps from p on leave lane p alone.
// The block is therefore assembled and factored ONCE and every member lane writes its own Y[row, c] = b / pivot and
// logd[row] = log(pivot): the bits of the ungrouped launch on the same (expanded) table, from |S| (|S| - 1) / 2 pairs instead
// of one triangle per member.  The totals are vecchia_sum_kernel's over the same per-row arrays.
//
// A pivot that fails at position q fails every member at a position >= q -- the rows the ungrouped launch reports --, and the
// smallest of them goes into the failure word by the same integer atomicMin.
//
// The workgroup is wider than the block: at 64 rows the LDS admits six workgroups per CU, and six single wavefronts leave the
// pair values -- the Bessel branch above all -- without anything to hide their latency behind.  The extra wavefronts take
// pairs, pass the barriers of the factorisation with nothing to do (a thread is a row only below nrows <= 64) and, in the
// value launch, end before the substitution, which has no barrier.
//
// Compile with -ffp-contract=off, like vecchia.hip: the products and sums stand as written.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "vecchia_block.hpp"

namespace cocons {

constexpr int VECCHIA_GROUP_FQ = 16;                   // the information: (member, direction) accumulators a thread keeps
static_assert(2 * GFAM % VECCHIA_GROUP_WAVES == 0, "the site sums are dealt evenly over the wavefronts");
static_assert(VECCHIA_GROUP_FQ == VECCHIA_FD && VECCHIA_GROUP_FQ % VECCHIA_G == 0, "a thread's accumulators go through "
              "vecchia_forward four at a time, and one wavefront can hold a whole group of directions of one member");
static_assert(COCONS_P_MAX * (VECCHIA_GROUP_FQ * VECCHIA_GROUP_WAVES / VECCHIA_G) <= VECCHIA_G * VECCHIA_GROUP_THREADS,
              "the members' sums u_p of a chunk fit the staging of the narrowest group");

// What every grouped launch opens with: the block's rows into nb, the phases up to the factor, the report of a failing pivot.
// row0: the rows below it are fixed and report nothing (the coefficient launch; 0 elsewhere).  SOLVES: the pivots go into the
// factor's diagonal, where the solves of the other wavefronts read them.  False: the block has nothing to give, the
// workgroup ends (all its threads alike).
template <int MODE, bool SITES, bool SOLVES>
__device__ __forceinline__ bool vecchia_group_open(const VecchiaGroupArgs &a, int blk, int row0, double *par, double *sp, double *tri,
                                                   int *nb, int &nrows, unsigned long long &members, double &piv_mine)
{
    const int lane = threadIdx.x, kb = a.kb, off = a.off[blk];
    nrows = a.off[blk + 1] - off;
    members = a.mask[blk];
    if (nrows < 1 || nrows > kb) return false;    // (a plan the host checked has none)
    // the rows ascend, so a block whose last row is fixed has nothing to give
    if (row0 > 0 && a.rows[off + nrows - 1] < row0) return false;
    if (lane < nrows) nb[lane] = a.rows[off + lane];
    __syncthreads();
    const int bad = vecchia_open_block<MODE, VECCHIA_GROUP_THREADS, SITES>(par, sp, tri, kb, nb, nrows, a.aosK, a.aosG, a.gr,
                                                                           a.nu_fixed, lane, piv_mine);
    if (bad >= 0) {
        // the members from position `bad` on fail; the last row of a block is a member and not fixed, so there is one
        unsigned long long late = members >> bad;
        while (row0 > 0 && late && nb[bad + __builtin_ctzll(late)] < row0) late &= late - 1;
        const int q = late ? bad + __builtin_ctzll(late) : nrows;
        if (lane == 0 && q < nrows) atomicMin(a.fail, nb[q] + 1);
        return false;
    }
    if (SOLVES && lane < nrows) tri[tri_at(lane, lane)] = piv_mine;
    __syncthreads();
    return true;
}

// The right-hand sides through the forward substitution in the first wavefront, VECCHIA_G at a time: lane r ends with
// b_r - sum_{j < r} C(r, j) y_j, j ascending, and every member lane stores Y[row, c] = that / pivot and log d.  A lane at or
// in front of step j takes no part in it: its value must not see a y_j that is not finite.
// each(b, c0): the numerators of the columns c0 .. in every lane.
template <class F>
__device__ __forceinline__ void vecchia_group_columns(const VecchiaGroupArgs &a, const double *tri, const int *nb, int nrows,
                                                      unsigned long long members, int lane, double piv_mine, F &&each)
{
    const bool member = lane < nrows && ((members >> lane) & 1ull);
    const int site = lane < nrows ? nb[lane] : 0, myrow = tri_at(lane, 0);
    for (int c0 = 0; lane < 64 && c0 < a.nb; c0 += VECCHIA_G) {
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
        each(b, c0);
    }
    if (member && a.logd) a.logd[site] = log(piv_mine);
}

// The members' backward solves s_p = L_{0..p}^-T e_p (N = 2: and h_p = L_{0..p}^-T N[p, 0..p), which takes the place of its
// right-hand side in nm) into row p of sm: member i (ascending) on wavefront i mod 4, lane = row -- the wavefront that owns
// the member is the only one that touches its rows.  vecchia_backward in its reciprocal form.
template <int N>
__device__ __forceinline__ void vecchia_group_solves(const double *tri, double *sm, double *nm, unsigned long long members, int nrows,
                                                     int wv, int ln)
{
    const double ipiv = ln < nrows ? 1.0 / tri[tri_at(ln, ln)] : 0.0;
    int rank = 0;
    for (unsigned long long rest = members; rest; rest &= rest - 1, ++rank) {
        if ((rank & (VECCHIA_GROUP_WAVES - 1)) != wv) continue;
        const int p = __builtin_ctzll(rest);
        double r[N], x[N];
#pragma unroll
        for (int g = 0; g < N; ++g) {
            r[g] = g == 0 ? (ln == p ? 1.0 : 0.0) : (ln < p ? nm[tri_at(p, ln)] : 0.0);
            x[g] = 0.0;
        }
        vecchia_backward<PIV_RECIPROCAL>(r, x, tri, ipiv, ln, p);
        if (ln <= p) sm[tri_at(p, ln)] = x[0];
        if (N > 1 && ln < p) nm[tri_at(p, ln)] = x[N - 1];
    }
}

// The value.
template <int MODE>
__global__ void __launch_bounds__(VECCHIA_GROUP_THREADS)
vecchia_group_value_kernel(VecchiaGroupArgs a)
{
    extern __shared__ double vecchia_group_lds[];
    const VecchiaValueLds L = vecchia_value_lds(a.kb, false);
    double *par = vecchia_group_lds + L.par, *tri = vecchia_group_lds + L.tri;
    int *nb = (int *)(vecchia_group_lds + L.nb);
    const int lane = threadIdx.x, blk = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    int nrows;
    unsigned long long members;
    double piv_mine;
    if (!vecchia_group_open<MODE, false, false>(a, blk, 0, par, nullptr, tri, nb, nrows, members, piv_mine)) return;
    if (lane >= 64) return;                        // (no barrier from here on)
    vecchia_group_columns(a, tri, nb, nrows, members, lane, piv_mine, [](const double (&)[VECCHIA_G], int) {});
}

// The coefficients: the members' backward solves s_p = L_{0..p}^-T e_p as vecchia_coef_kernel runs them on the
// leading (p + 1) x (p + 1) sub-block -- vecchia_backward in its dividing form -- and every s_p goes straight into its row's
// record of launch_vecchia_coefs.  The factor's bits are the ungrouped leading sub-block's, the solve reads nothing else, so
// the records are the bits of the ungrouped launch on the same table.  The members are dealt over the four wavefronts by
// rank, and a wavefront solves VECCHIA_G of its members at a time: they share the read of the factor's row and give the
// shuffles four independent chains.
template <int MODE>
__global__ void __launch_bounds__(VECCHIA_GROUP_THREADS)
vecchia_group_coef_kernel(VecchiaGroupArgs a)
{
    extern __shared__ double vecchia_group_lds[];
    const VecchiaValueLds L = vecchia_value_lds(a.kb, false);
    double *par = vecchia_group_lds + L.par, *tri = vecchia_group_lds + L.tri;
    int *nb = (int *)(vecchia_group_lds + L.nb);
    const int lane = threadIdx.x, blk = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    int nrows;
    unsigned long long members;
    double piv_mine;
    if (!vecchia_group_open<MODE, false, true>(a, blk, a.row0, par, nullptr, tri, nb, nrows, members, piv_mine)) return;
    // No barrier from here on: a wavefront that carries no member's solve falls through the loop and ends.  Member i
    // (ascending, among those whose row is not fixed) is wavefront i mod 4's, lane = row.
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
        vecchia_backward<PIV_DIVIDE>(rs, sv, tri, pivl, ln, pg[cnt - 1], pg);
        const int m = (int)a.ldc - 1;
#pragma unroll
        for (int g = 0; g < VECCHIA_G; ++g) {
            if (pg[g] < 0) continue;
            double *rec = a.coef + (size_t)nb[pg[g]] * a.ldc;
            if (ln < m) rec[ln] = ln < pg[g] ? sv[g] : 0.0;
            if (ln == pg[g]) rec[m] = sv[g];
        }
    }
}

// The gradient: the value's phases, then the block's share of the gradient.  The member at position p is 4s's
// block on the leading p + 1 rows, so the block's weights are the members' weights summed:
//   W_log = nb sum_p s_p s_p',   W_quad = sum_p [ -N_pp s_p s_p' - (h_p s_p' + s_p h_p') ],   N = sum_c w_c w_c',
// with s_p = L^-T e_p (row p of L^-1) and h_p = L_{0..p}^-T N[p, 0..p).  The substitution leaves N's member rows in LDS, the
// members' backward solves are dealt over the four wavefronts, and every pair's partials are evaluated ONCE by one of the
// VECCHIA_GROUP_THREADS threads and weighted with the two sums over the members, ascending.  One record per block.
template <int MODE>
__global__ void __launch_bounds__(VECCHIA_GROUP_THREADS)
vecchia_group_grad_kernel(VecchiaGroupArgs a)
{
    extern __shared__ double vecchia_group_lds[];
    constexpr int T = VECCHIA_GROUP_THREADS;
    const int kb = a.kb;
    const VecchiaGradLds L = vecchia_grad_lds(kb, true);
    double *par = vecchia_group_lds + L.par, *tri = vecchia_group_lds + L.tri, *sm = vecchia_group_lds + L.sm;
    double *nm = vecchia_group_lds + L.nm, *sp = vecchia_group_lds + L.sp, *ys = vecchia_group_lds + L.v1;
    double *uv = vecchia_group_lds + L.v2, *gs = vecchia_group_lds + L.gs, *red = vecchia_group_lds + L.red;
    int *nb = (int *)(vecchia_group_lds + L.nb);
    const int lane = threadIdx.x, wv = lane >> 6, ln = lane & 63;
    const int blk = a.blk0 + (a.order ? a.order[blockIdx.x] : (int)blockIdx.x);
    const int nz = min(a.off[blk + 1] - a.off[blk], kb);
    for (int e = lane; e < nz * (nz + 1) / 2; e += T) nm[e] = 0.0;     // (the open's barriers stand before the first use)
    int nrows;
    unsigned long long members;
    double piv_mine;
    if (!vecchia_group_open<MODE, true, true>(a, blk, 0, par, sp, tri, nb, nrows, members, piv_mine)) return;
    const int npairs = nrows * (nrows - 1) / 2;
    // every lane j ends with the numerator of w_c[j], so N[p, j] = sum_c w_c[p] w_c[j] of the member rows p >= j and
    // sum_c w_c[p] are formed on the way, the columns ascending (the other wavefronts go on to the barrier)
    double ysum = 0.0;
    vecchia_group_columns(a, tri, nb, nrows, members, lane, piv_mine, [&](const double (&b)[VECCHIA_G], int c0) {
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
    });
    if (lane < nrows) ys[lane] = ysum;
    __syncthreads();
    vecchia_group_solves<2>(tri, sm, nm, members, nrows, wv, ln);
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
    // thread (row ln, wavefront wv) keeps NACC of the row's 2 GFAM site sums, q = wv NACC + i: the log-determinant's share
    // of family q below GFAM, the quadratic forms' of family q - GFAM from there on
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
    // The pair walk: T pairs a pass, one per thread (the order of the assembly), each pair's partials evaluated once and
    // staged with 2 W_log and 2 W_quad; then thread (a, wv) adds what the pass holds for its site by vecchia_row_pairs' rule.
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
            auto add = [&](int side, int slot) {
                const double w = stg[wsel * T + slot];
#pragma unroll
                for (int i = 0; i < NACC; ++i) acc[i] += w * stg[(side + f0 + i) * T + slot];
            };
            vecchia_row_pairs(ln, t0, min(t0 + T, npairs), [&](int slot, int) { add(GFAM, slot); },
                              [&](int slot, int) { add(0, slot); });
        }
        __syncthreads();
    }
    if (ln < nrows) {
#pragma unroll
        for (int i = 0; i < NACC; ++i) gs[(q0 + i) * kb + ln] = acc[i];
    }
    // the global-range sums: a fixed butterfly per wavefront, the wavefronts' shares added in their order
    glob_l = vecchia_wave_sum(glob_l);
    glob_q = vecchia_wave_sum(glob_q);
    if (ln == 0) { red[wv] = glob_l; red[VECCHIA_GROUP_WAVES + wv] = glob_q; }
    __syncthreads();
    // the record, at the block's id: the site sums contracted with X over the block's rows, ascending
    const int p = a.p, b = blk - a.blk0;
    for (int o = lane; o < (2 * GFAM + 1) * p; o += T) {
        const int q = o / p, kx = o % p;
        const double s = vecchia_dot_x(q < 2 * GFAM ? gs + q * kb : uv, nrows, nb, a.X, a.ldx, kx);
        a.rec[(size_t)(q < 2 * GFAM ? o : 2 * GFAM * p + 2 + kx) * a.ldr + b] = s;
    }
    if (lane == 0) {
        double gl = red[0], gq = red[VECCHIA_GROUP_WAVES];
        for (int w = 1; w < VECCHIA_GROUP_WAVES; ++w) { gl += red[w]; gq += red[VECCHIA_GROUP_WAVES + w]; }
        a.rec[(size_t)(2 * GFAM * p) * a.ldr + b] = gl;
        a.rec[(size_t)(2 * GFAM * p + 1) * a.ldr + b] = gq;
    }
}

// The information: the members' backward solves without h, then the block's share of the expected
// information.  The member at position p is 4t's block on the leading p + 1 rows: with q_{a,p} = C_a[0..p, 0..p] s_p and
// g_{a,p} = L_{0..p}^-1 q_{a,p} it gives sum_{j < p} g_a[j] g_b[j] + g_a[p] g_b[p] / 2, and the block the sum over its
// members.  The factor stays in LDS for the forward solves; every pair's partials are evaluated once per walk and serve all
// the members of a chunk and all the directions of a group.  One record per block.
template <int MODE>
__global__ void __launch_bounds__(VECCHIA_GROUP_THREADS)
vecchia_group_fisher_kernel(VecchiaGroupArgs a)
{
    extern __shared__ double vecchia_group_lds[];
    constexpr int T = VECCHIA_GROUP_THREADS;
    const int kb = a.kb, p = a.p, ndir = a.ndir, gw = a.gd, mc = a.mc;
    const VecchiaFisherLds L = vecchia_fisher_lds(kb, ndir, gw, mc, true);
    double *par = vecchia_group_lds + L.par, *tri = vecchia_group_lds + L.tri, *sm = vecchia_group_lds + L.sm;
    double *sp = vecchia_group_lds + L.sp, *wts = vecchia_group_lds + L.wts, *stg = vecchia_group_lds + L.stg;
    double *gall = vecchia_group_lds + L.gall;
    int *mpos = (int *)(vecchia_group_lds + L.sv), *nb = (int *)(vecchia_group_lds + L.nb);
    const int lane = threadIdx.x, wv = lane >> 6, ln = lane & 63;
    const int blk = a.blk0 + (a.order ? a.order[blockIdx.x] : (int)blockIdx.x), b = blk - a.blk0;
    int nrows;
    unsigned long long members;
    double piv_mine;
    if (!vecchia_group_open<MODE, true, true>(a, blk, 0, par, sp, tri, nb, nrows, members, piv_mine)) return;
    const int npairs = nrows * (nrows - 1) / 2, ng = ndir * (ndir + 1) / 2, nmem = __popcll(members);
    if (lane < nrows && ((members >> lane) & 1ull)) mpos[__popcll(members & ((1ull << lane) - 1ull))] = lane;
    vecchia_group_solves<1>(tri, sm, nullptr, members, nrows, wv, ln);
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
            const int pp = mpos[m0 + e / p];
            stg[e] = vecchia_dot_x(sm + tri_at(pp, 0), pp + 1, nb, a.X, a.ldx, e % p);
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
            vecchia_site_weights<T>(wts, kb, nrows, nb, a.X, a.ldx, p, a.dirs, d0, gd, lane);
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
                vecchia_stage_dir_entries<MODE, T>(stg, wts, par, sp, kb, a.gr, a.nu_fixed, a.smooth_free, a.dirs, p, d0, gd,
                                                   t0 + lane, npairs, lane);
                __syncthreads();
                if (ln < nrows) {
                    // member p takes the pairs with r <= p: `top` is the pair's later row
                    auto add = [&](int slot, int other, int top) {
#pragma unroll
                        for (int k = 0; k < NB; ++k) {
                            if (pm[k] < top) continue;
                            const double so = sm[tri_at(pm[k], 0) + other];
#pragma unroll
                            for (int g = 0; g < VECCHIA_G; ++g)
                                if (db[k] + g < gd) q[k * VECCHIA_G + g] += stg[(db[k] + g) * T + slot] * so;
                        }
                    };
                    vecchia_row_pairs(ln, t0, min(t0 + T, npairs), [&](int slot, int c) { add(slot, c, ln); },
                                      [&](int slot, int r) { add(slot, r, r); });
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
        // ascending, the rows ascending within a member -- kept in the record from chunk to chunk, so it does not depend on mc
        for (int o = lane; o < ng; o += T) {
            int ra, cb;
            tri_pair(o, ra, cb);       // (the strict triangle's numbering of (a + 1, b))
            double *dst = a.rec + (size_t)o * a.ldr + b;
            double s = m0 ? *dst : 0.0;
            for (int mi = 0; mi < cm; ++mi)
                s = vecchia_gram_add(s, gall + ((size_t)mi * ndir + ra - 1) * kb, gall + ((size_t)mi * ndir + cb) * kb,
                                     mpos[m0 + mi]);
            *dst = s;
        }
        __syncthreads();               // (the next chunk writes stg and gall)
    }
}

// kb <= 64: the value's and the coefficients' LDS is at most 23 552 bytes, no attribute needed; the gradient's at most 78 144
void launch_vecchia_group_blocks(int mode, const VecchiaGroupArgs &a, hipStream_t s)
{
    if (a.blocks <= 0) return;
    vecchia_with_mode(mode, [&](auto M) {
        vecchia_launch_kernel(vecchia_group_value_kernel<decltype(M)::value>, a, a.blocks, VECCHIA_GROUP_THREADS,
                              vecchia_lds_bytes(a.kb - 1, false), s);
    });
}

void launch_vecchia_group_coefs(int mode, const VecchiaGroupArgs &a, hipStream_t s)
{
    if (a.blocks <= 0) return;
    vecchia_with_mode(mode, [&](auto M) {
        vecchia_launch_kernel(vecchia_group_coef_kernel<decltype(M)::value>, a, a.blocks, VECCHIA_GROUP_THREADS,
                              vecchia_lds_bytes(a.kb - 1, false), s);
    });
}

size_t vecchia_group_grad_lds_bytes(int kb) { return vecchia_grad_lds(kb, true).bytes; }

void launch_vecchia_group_grad_blocks(int mode, const VecchiaGroupArgs &a, hipStream_t s)
{
    if (a.blocks <= 0) return;
    vecchia_with_mode(mode, [&](auto M) {
        static std::atomic<unsigned long long> attr_done{0};           // (one per instantiation)
        vecchia_launch_kernel(vecchia_group_grad_kernel<decltype(M)::value>, a, a.blocks, VECCHIA_GROUP_THREADS,
                              vecchia_group_grad_lds_bytes(a.kb), s, &attr_done, vecchia_group_grad_lds_bytes(64));
    });
}

// The shape of an information launch: a thread keeps VECCHIA_GROUP_FQ = 16 accumulators and the four wavefronts 64 slots, so
// gd directions a group leave 64 / gd members a chunk.  gd is the smallest of 4, 8, 16 that holds ndir (16 from ndir = 9 on:
// the fewest pair walks, ceil(members / mc) ceil(ndir / gd)), mc = 64 / gd; while the LDS is above VECCHIA_FISHER_LDS_MAX first
// mc is halved (gall shrinks), then gd (wts and stg shrink).
size_t vecchia_group_fisher_lds_bytes(int kb, int ndir, int gd, int mc) { return vecchia_fisher_lds(kb, ndir, gd, mc, true).bytes; }

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

void launch_vecchia_group_fisher_blocks(int mode, const VecchiaGroupArgs &a, hipStream_t s)
{
    if (a.blocks <= 0) return;
    vecchia_with_mode(mode, [&](auto M) {
        static std::atomic<unsigned long long> attr_done{0};           // (one per instantiation)
        vecchia_launch_kernel(vecchia_group_fisher_kernel<decltype(M)::value>, a, a.blocks, VECCHIA_GROUP_THREADS,
                              vecchia_group_fisher_lds_bytes(a.kb, a.ndir, a.gd, a.mc), s, &attr_done, VECCHIA_FISHER_LDS_MAX);
    });
}

}  // namespace cocons
