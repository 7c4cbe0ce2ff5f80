// band_plan.hpp -- the host-side book-keeping of a taper handle's band factor, in ONE place: the envelope rule (which tiles of
// the factor a pattern can fill) and the packed layout of the factor's tiles that every entry holding or sweeping a band factor
// uses (tapered kriging, the tapered information), and the bucket sort by tile column that tapered kriging scatters a chunk's
// entries into its ring by.  Host only, standard headers only: tests/band_plan_main.cpp compiles it with a plain C++17
// compiler and tests/test_taper_envelope_cases.py holds it against restatements in numpy.
#pragma once
#include <climits>
#include <vector>

namespace cocons {

// The tile envelope of a pattern: hi[c] = one past the last 128-row tile of tile column c that the factor can fill, and
// maxband = max_c (hi[c] - c).  rowpointers / colindices: the 1-based CSR of the full pattern in the handle's order.
struct BandEnvelope { std::vector<int> hi; int maxband = 0; };

inline BandEnvelope band_envelope(int n, const int *rowpointers, const int *colindices, int tile)
{
    const int nt = (n + tile - 1) / tile;
    // the raw skyline: row i of the factor is non-zero from its first stored column on
    std::vector<int> raw(nt);
    for (int c = 0; c < nt; ++c) raw[c] = c + 1;
    for (int i = 0; i < n; ++i) {
        int first = i;
        for (int w = rowpointers[i] - 1; w < rowpointers[i + 1] - 1; ++w) if (colindices[w] - 1 < first) first = colindices[w] - 1;
        const int ti = i / tile;
        for (int c = first / tile; c <= ti; ++c) if (raw[c] < ti + 1) raw[c] = ti + 1;
    }
    // The schedule works on 256-column blocks and updates the square [t, hb) x [t, hb) with a block's panel: make the bound
    // per block (both tile columns, at least the next diagonal block) and monotone, so that every tile an update touches lies
    // inside the bound of its own column -- which is what gets zeroed.
    BandEnvelope e; e.hi.resize(nt);
    int run = 0;
    for (int c = 0; c < nt; ++c) {
        const int k = c & ~1;
        int hb = raw[k];
        if (k + 1 < nt && raw[k + 1] > hb) hb = raw[k + 1];
        const int need = k + 4 < nt ? k + 4 : nt;
        if (hb < need) hb = need;
        if (hb > nt) hb = nt;
        if (hb > run) run = hb;
        e.hi[c] = run;
        if (run - c > e.maxband) e.maxband = run - c;
    }
    return e;
}

// The packed layout of a band factor on nt tile columns: tile (I, J), J <= I < hi[J], is tile toff[J] + (I - J) of the packed
// buffer, a ring of W tile columns holds every tile row a column reaches.  hib / toffb: the same for the flipped factor
// M = F L' F (rows and columns reversed, transposed) of the backward sweep: hib[J'] = nt - the first tile column that reaches
// tile row nt - 1 - J'.  toff and toffb have nt + 1 entries and end in the same count (the same tiles from the other end).
struct BandPlan { int nt = 0, W = 0; std::vector<int> hi, hib, toff, toffb; };

// hi: the handle's envelope with its maxband, or null when it has none -- then every column reaches the last tile row
// (hi[c] = nt, W = nt).  Returns null, or what is wrong with the envelope (the plan is then not to be used).
inline const char *band_plan(int nt, const int *hi, int maxband, BandPlan &pl)
{
    pl.nt = nt; pl.W = hi ? maxband : nt;
    pl.hi = hi ? std::vector<int>(hi, hi + nt) : std::vector<int>((size_t)nt, nt);
    pl.hib.assign((size_t)nt, 0); pl.toff.assign((size_t)nt + 1, 0); pl.toffb.assign((size_t)nt + 1, 0);
    for (int J = nt - 1, lo = nt - 1; J >= 0; --J) {
        if (lo > J) lo = J;
        while (lo > 0 && pl.hi[lo - 1] > J) --lo;
        pl.hib[nt - 1 - J] = nt - lo;
    }
    for (int J = 0; J < nt; ++J) {
        const long long a = (long long)pl.toff[J] + (pl.hi[J] - J), b = (long long)pl.toffb[J] + (pl.hib[J] - J);
        if (a > INT_MAX || b > INT_MAX) return "the envelope holds too many tiles";
        pl.toff[J + 1] = (int)a; pl.toffb[J + 1] = (int)b;
    }
    return pl.toffb[nt] == pl.toff[nt] ? nullptr : "the envelope is not monotone";
}

// The entries of rows [row0, row0 + nrows) of a caller's pattern (ci / rp: its 1-based CSR, already checked) in the handle's
// order of the columns -- inv[caller's column] = position --, bucketed by tile column for the ring solve of tapered kriging.
// With e0 = rp[row0] - 1 the chunk's first entry and w counted from it:
//   hci[w]              1-based position of entry w's column;
//   boff[I], boff[I+1]  (nt + 1 entries) the bucket of tile column I in hdst / hsrc, which for its k-th place hold
//   hsrc[k]             the entry w, and
//   hdst[k]             where it goes in the tile column's slot: (row - row0) + (position % tile) * stride, stride the slot's
//                       leading dimension (>= nrows).
// A counting sort that walks the rows in order, so a bucket keeps the rows' order and, within a row, the caller's.  (The tile
// edge is a template argument: two divisions per entry, which the compiler turns into shifts.)
template <int tile>
void band_buckets(int nt, const int *inv, const int *ci, const int *rp, int row0, int nrows, int stride,
                  std::vector<int> &hci, std::vector<int> &hdst, std::vector<int> &hsrc, std::vector<int> &boff)
{
    const int e0 = rp[row0] - 1, ne = rp[row0 + nrows] - 1 - e0;
    hci.resize((size_t)ne); hdst.resize((size_t)ne); hsrc.resize((size_t)ne);
    boff.assign((size_t)nt + 1, 0);
    for (int w = 0; w < ne; ++w) {
        const int c = inv[ci[e0 + w] - 1];
        hci[w] = c + 1;
        ++boff[c / tile + 1];
    }
    std::vector<int> fill((size_t)nt);
    for (int I = 0; I < nt; ++I) { boff[I + 1] += boff[I]; fill[I] = boff[I]; }
    for (int i = 0; i < nrows; ++i)
        for (int w = rp[row0 + i] - 1 - e0; w < rp[row0 + i + 1] - 1 - e0; ++w) {
            const int c = hci[w] - 1, k = fill[c / tile]++;
            hdst[k] = i + (c % tile) * stride;
            hsrc[k] = w;
        }
}

}  // namespace cocons
