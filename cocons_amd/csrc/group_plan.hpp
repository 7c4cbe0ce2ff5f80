// group_plan.hpp -- grouped Vecchia blocks (vecchia_group.hip), in ONE place for the host entries, the closure
// check of cocons_vecchia_set_groups and the stand-alone program of tests/group_plan_main.cpp: the greedy grouping rule, the
// sets S of a partition, the expanded table and the device plan.  Integers only -- tests/group_reference.py restates every
// function in numpy and the two agree integer for integer.  Standard headers only.
//
// A block B is a set of member rows; S(B) is the union of its members and of all their table neighbours.  The rule: every row
// starts as a block of its own; the rows are visited in ascending order, and for each neighbour j of row i, in the order the
// caller's row lists them (zeros skipped), the blocks A = block(i) and B = block(j) are merged when
//     A != B,   u = |S(A) u S(B)| <= max_rows   and   u^2 < |S(A)|^2 + |S(B)|^2
// (Guinness 2018: the merged block's squared size is below the sum of the two).  A row that is never merged keeps its own
// S, whatever max_rows is; every block that a merge made has |S| <= max_rows.
//
// A member that stands at position p of its block's ascending rows conditions on the positions 0 .. p - 1: its row of the
// expanded table.  Because every neighbour of a member is an earlier row, the last row of a block is always a member.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace cocons {

constexpr int GROUP_ROWS_MAX = 64;     // rows of a block: one wavefront, lane = row; the expanded table has m <= 63

// A neighbour table in one of its two layouts.  caller: rows x m column-major, 1-based, 0 = none (cocons_fit_create_vecchia's
// nn).  device: rows x m row after row, 0-based, -1 = none (VecchiaState::nbr).  each(i, f): f(j) for the 0-based neighbours of
// row i in stored order.
struct GroupTable {
    const int *p = nullptr;
    size_t n = 0;
    int m = 0;
    bool device = false;
    template <class F> void each(size_t i, F f) const
    {
        for (int j = 0; j < m; ++j) {
            const int v = device ? p[i * (size_t)m + j] : p[i + (size_t)j * n] - 1;
            if (v >= 0) f(v);
        }
    }
    int count(size_t i) const
    {
        int k = 0;
        each(i, [&](int) { ++k; });
        return k;
    }
};

// pairs the ungrouped schedule evaluates on the table: (k + 1) k / 2 for a row of k neighbours
inline long long group_pairs_ungrouped(const GroupTable &t)
{
    long long s = 0;
    for (size_t i = 0; i < t.n; ++i) { const long long k = t.count(i); s += (k + 1) * k / 2; }
    return s;
}

// |a u b| of two ascending lists without repeats; out (may be null): the union
inline int group_union(const std::vector<int> &a, const std::vector<int> &b, std::vector<int> *out)
{
    size_t x = 0, y = 0;
    int u = 0;
    if (out) out->clear();
    while (x < a.size() || y < b.size()) {
        int v;
        if (y >= b.size() || (x < a.size() && a[x] < b[y])) v = a[x++];
        else if (x >= a.size() || b[y] < a[x]) v = b[y++];
        else { v = a[x]; ++x; ++y; }
        if (out) out->push_back(v);
        ++u;
    }
    return u;
}

// The greedy rule on a valid table (every neighbour an earlier row, no neighbour twice in a row).  group[n]: 0-based block
// ids, the blocks numbered by their smallest member, ascending.  Returns the number of blocks.
inline int group_greedy(const GroupTable &t, int max_rows, int *group)
{
    const size_t n = t.n;
    std::vector<int> blk(n);
    std::vector<std::vector<int>> S(n), members(n);
    std::vector<int> un;
    for (size_t i = 0; i < n; ++i) {
        blk[i] = (int)i;
        members[i].assign(1, (int)i);
        std::vector<int> &own = S[i];
        own.assign(1, (int)i);
        t.each(i, [&](int j) { own.push_back(j); });
        std::sort(own.begin(), own.end());
        t.each(i, [&](int j) {
            const int A = blk[i], B = blk[(size_t)j];
            if (A == B) return;
            const long long a = (long long)S[(size_t)A].size(), b = (long long)S[(size_t)B].size();
            const long long u = group_union(S[(size_t)A], S[(size_t)B], nullptr);
            if (u > max_rows || u * u >= a * a + b * b) return;
            group_union(S[(size_t)A], S[(size_t)B], &un);
            S[(size_t)A] = un;
            for (int r : members[(size_t)B]) { blk[(size_t)r] = A; members[(size_t)A].push_back(r); }
            std::vector<int>().swap(S[(size_t)B]);
            std::vector<int>().swap(members[(size_t)B]);
        });
    }
    std::vector<int> id(n, -1);
    int next = 0;
    for (size_t i = 0; i < n; ++i) {
        int &l = id[(size_t)blk[i]];
        if (l < 0) l = next++;
        group[i] = l;
    }
    return next;
}

// The round rule: a grouping that is a function of the table's neighbour SETS alone, stated so that a device
// can run it -- every round reads only the state at its start.  A block's id is its smallest member.  One round:
//   1. every live block A proposes the eligible candidate B (a block that holds a neighbour of a member of A; eligible: the
//      greedy rule's test, u <= max_rows and u^2 < a^2 + b^2) of the largest gain g = a^2 + b^2 - u^2, ties to the smaller id;
//      key(A) = (8192 - g) << 32 | A;
//   2. best(X) = the smallest key(A) over the proposing A with A = X or prop(A) = X;
//   3. the edge A -> prop(A) = B is realised when best(A) = best(B) = key(A); realised edges share no block, and each merges
//      its two blocks into the smaller id.
// The rounds end with the first round without a proposal, or after max_rounds rounds (0: GROUP_ROUNDS_MAX).
constexpr int GROUP_ROUNDS_MAX = 256;
constexpr unsigned long long GROUP_NO_KEY = ~0ull;

constexpr unsigned long long group_key(int a, int b, int u, int id)    // (constexpr: the kernels of group.hip call it too)
{
    return (unsigned long long)(8192 - (a * a + b * b - u * u)) << 32 | (unsigned)id;
}

// The state of the round rule after its rounds: blk[n] (row -> id of its block) and S (per id; empty once absorbed).
// Returns the rounds that merged something.
inline int group_rounds_state(const GroupTable &t, int max_rows, int max_rounds, std::vector<int> &blk,
                              std::vector<std::vector<int>> &S)
{
    const size_t n = t.n;
    const int cap = max_rounds > 0 ? max_rounds : GROUP_ROUNDS_MAX;
    blk.resize(n);
    S.assign(n, std::vector<int>());
    std::vector<int> live(n), prop(n, -1), seen, un;
    std::vector<unsigned long long> key(n, GROUP_NO_KEY), best(n, GROUP_NO_KEY);
    for (size_t i = 0; i < n; ++i) {
        blk[i] = live[i] = (int)i;
        S[i].assign(1, (int)i);
        t.each(i, [&](int j) { S[i].push_back(j); });
        std::sort(S[i].begin(), S[i].end());
    }
    int rounds = 0;
    while (rounds < cap) {
        bool any = false;
        for (int A : live) {
            key[(size_t)A] = best[(size_t)A] = GROUP_NO_KEY;
            prop[(size_t)A] = -1;
        }
        for (int A : live) {
            const std::vector<int> &sa = S[(size_t)A];
            const int a = (int)sa.size();
            if (a > max_rows) continue;
            // every row of S(A) that is no member is a neighbour of one: the candidates are the blocks of S(A)'s rows
            seen.clear();
            unsigned long long kb = GROUP_NO_KEY;      // (8192 - g) << 32 | B: the smallest is the largest gain, then the smaller id
            for (int s : sa) {
                const int B = blk[(size_t)s];
                if (B == A || std::find(seen.begin(), seen.end(), B) != seen.end()) continue;
                seen.push_back(B);
                const int b = (int)S[(size_t)B].size();
                if (b > max_rows) continue;
                const int u = group_union(sa, S[(size_t)B], nullptr);
                if (u > max_rows || u * u >= a * a + b * b) continue;
                kb = std::min(kb, group_key(a, b, u, B));
            }
            if (kb == GROUP_NO_KEY) continue;
            any = true;
            prop[(size_t)A] = (int)(kb & 0xffffffffull);
            key[(size_t)A] = (kb >> 32) << 32 | (unsigned)A;
        }
        if (!any) break;
        for (int A : live)
            if (prop[(size_t)A] >= 0) {
                best[(size_t)A] = std::min(best[(size_t)A], key[(size_t)A]);
                best[(size_t)prop[(size_t)A]] = std::min(best[(size_t)prop[(size_t)A]], key[(size_t)A]);
            }
        for (int A : live) {
            const int B = prop[(size_t)A];
            if (B < 0 || best[(size_t)A] != key[(size_t)A] || best[(size_t)B] != key[(size_t)A]) continue;
            const int lo = std::min(A, B), hi = std::max(A, B);
            group_union(S[(size_t)lo], S[(size_t)hi], &un);
            for (int s : S[(size_t)hi]) if (blk[(size_t)s] == hi) blk[(size_t)s] = lo;
            S[(size_t)lo] = un;
            std::vector<int>().swap(S[(size_t)hi]);
        }
        live.erase(std::remove_if(live.begin(), live.end(), [&](int A) { return blk[(size_t)A] != A; }), live.end());
        ++rounds;
    }
    return rounds;
}

// group[n]: the labels of the round rule's partition, the blocks numbered by their smallest member, ascending, as
// group_greedy's are; *rounds_run (may be null): the rounds that merged something.  Returns the number of blocks.
inline int group_rounds(const GroupTable &t, int max_rows, int max_rounds, int *group, int *rounds_run)
{
    std::vector<int> blk;
    std::vector<std::vector<int>> S;
    const int rounds = group_rounds_state(t, max_rows, max_rounds, blk, S);
    if (rounds_run) *rounds_run = rounds;
    std::vector<int> id(t.n, -1);
    int next = 0;
    for (size_t i = 0; i < t.n; ++i) {
        int &l = id[(size_t)blk[i]];
        if (l < 0) l = next++;
        group[i] = l;
    }
    return next;
}

// What the kernel walks: block b holds the rows rows[off[b] .. off[b + 1]) -- S(b), ascending, 0-based --, bit p of mask[b]
// says whether the row at position p is a member, and order[] lists the blocks largest first (ties: the smaller id first),
// the sequence a launch deals them to its workgroups in.  The blocks are numbered by their smallest member, ascending,
// whatever labels the partition came with.
struct GroupPlan {
    std::vector<int> off, rows, order;
    std::vector<unsigned long long> mask;
    std::vector<int> block, pos;       // per row: its block, and its position in that block's rows
    int blocks = 0, maxrows = 0, longest = 0;      // longest: the largest position of a member = the longest expanded row
    long long sum_rows = 0, pairs = 0;             // over the blocks: rows, and rows (rows - 1) / 2
};

// The plan of ANY partition `group` (labels in 0 .. n - 1) of the table's rows.  0, or the 1-based smallest member of the first
// block (in the plan's numbering) with |S| > GROUP_ROWS_MAX -- the plan is then not usable --, or -(i + 1) for the first
// row i whose label is out of range.
inline int group_plan(const GroupTable &t, const int *group, GroupPlan &pl)
{
    const size_t n = t.n;
    pl = GroupPlan();
    std::vector<int> canon(n, -1);
    pl.block.assign(n, 0);
    pl.pos.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (group[i] < 0 || (size_t)group[i] >= n) return -(int)(i + 1);
        int &c = canon[(size_t)group[i]];
        if (c < 0) c = pl.blocks++;
        pl.block[i] = c;
    }
    // the members by block (a counting sort keeps them ascending)
    std::vector<int> moff((size_t)pl.blocks + 1, 0), mem(n);
    for (size_t i = 0; i < n; ++i) ++moff[(size_t)pl.block[i] + 1];
    for (int b = 0; b < pl.blocks; ++b) moff[(size_t)b + 1] += moff[(size_t)b];
    {
        std::vector<int> cur(moff.begin(), moff.end() - 1);
        for (size_t i = 0; i < n; ++i) mem[(size_t)cur[(size_t)pl.block[i]]++] = (int)i;
    }
    pl.off.assign(1, 0);
    pl.mask.reserve((size_t)pl.blocks);
    std::vector<int> s;
    for (int b = 0; b < pl.blocks; ++b) {
        s.clear();
        for (int e = moff[(size_t)b]; e < moff[(size_t)b + 1]; ++e) {
            const int i = mem[(size_t)e];
            s.push_back(i);
            t.each((size_t)i, [&](int j) { s.push_back(j); });
        }
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        if ((int)s.size() > GROUP_ROWS_MAX) return mem[(size_t)moff[(size_t)b]] + 1;
        unsigned long long mask = 0;
        for (size_t q = 0; q < s.size(); ++q)
            if (pl.block[(size_t)s[q]] == b) {
                mask |= 1ull << q;
                pl.pos[(size_t)s[q]] = (int)q;
                pl.longest = std::max(pl.longest, (int)q);
            }
        pl.rows.insert(pl.rows.end(), s.begin(), s.end());
        pl.off.push_back((int)pl.rows.size());
        pl.mask.push_back(mask);
        const long long k = (long long)s.size();
        pl.maxrows = std::max(pl.maxrows, (int)k);
        pl.sum_rows += k;
        pl.pairs += k * (k - 1) / 2;
    }
    // largest first: a counting sort by rows, stable in the block id
    std::vector<int> start((size_t)GROUP_ROWS_MAX + 2, 0);
    for (int b = 0; b < pl.blocks; ++b) ++start[(size_t)(GROUP_ROWS_MAX - (pl.off[(size_t)b + 1] - pl.off[(size_t)b])) + 1];
    for (int k = 0; k <= GROUP_ROWS_MAX; ++k) start[(size_t)k + 1] += start[(size_t)k];
    pl.order.assign((size_t)pl.blocks, 0);
    for (int b = 0; b < pl.blocks; ++b)
        pl.order[(size_t)start[(size_t)(GROUP_ROWS_MAX - (pl.off[(size_t)b + 1] - pl.off[(size_t)b]))]++] = b;
    return 0;
}

// The expanded table of a plan: n x m_out column-major, 1-based, zero padded; member i gets {s in S(block(i)) : s < i},
// ascending.  m_out >= max(pl.longest, 1) is the caller's to check.
inline void group_table(const GroupPlan &pl, size_t n, int m_out, int *nn_out)
{
    std::fill(nn_out, nn_out + n * (size_t)m_out, 0);
    for (size_t i = 0; i < n; ++i) {
        const int *r = pl.rows.data() + pl.off[(size_t)pl.block[i]];
        for (int j = 0; j < pl.pos[i]; ++j) nn_out[i + (size_t)j * n] = r[j] + 1;
    }
}

// Whether the table is closed under the plan made from it: every member's stored row must be {s in S(block) : s < i}.  The
// stored neighbours are earlier rows of S by construction, so the row is closed exactly when it holds as many neighbours as
// the member has rows in front of it.  0, or the 1-based first row that is not; *have, *need: the two counts of that row.
inline int group_closed(const GroupTable &t, const GroupPlan &pl, int *have, int *need)
{
    for (size_t i = 0; i < t.n; ++i) {
        const int k = t.count(i);
        if (k != pl.pos[i]) {
            if (have) *have = k;
            if (need) *need = pl.pos[i];
            return (int)(i + 1);
        }
    }
    return 0;
}

}  // namespace cocons
