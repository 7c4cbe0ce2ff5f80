// The library's grouping rule, plan, expanded table and closure check (cocons_amd/csrc/group_plan.hpp) on the CPU, for
// tests/test_group_plan.py.  Input file: n, m, max_rows and have_group, then the n x m table row by row (1-based, 0 = none)
// and, with have_group = 1, n block labels; without them the greedy rule makes the labels.  Output: one line per table, its
// name first.  `status` is group_plan's return; the plan's lines and the expanded table follow only when it is 0.
#include <cstdio>
#include <vector>

#include "group_plan.hpp"

template <class T> static void print(const char *name, const std::vector<T> &v)
{
    printf("%s", name);
    for (T x : v) printf(" %llu", (unsigned long long)x);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n = 0, m = 0, max_rows = 0, have = 0;
    if (fscanf(fh, "%d %d %d %d", &n, &m, &max_rows, &have) != 4 || n < 1 || m < 1 || max_rows < 2 || max_rows > 64) {
        fprintf(stderr, "bad n, m, max_rows or have_group\n");
        return 2;
    }
    std::vector<int> nn((size_t)n * m), group((size_t)n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            int v = 0;
            if (fscanf(fh, "%d", &v) != 1 || v < 0 || v > i) { fprintf(stderr, "bad table entry in row %d\n", i + 1); return 2; }
            nn[(size_t)i + (size_t)j * n] = v;
        }
    if (have)
        for (int &g : group) if (fscanf(fh, "%d", &g) != 1) { fprintf(stderr, "short labels\n"); return 2; }
    fclose(fh);
    cocons::GroupTable t;
    t.p = nn.data(); t.n = (size_t)n; t.m = m;
    if (!have) cocons::group_greedy(t, max_rows, group.data());
    print("group", group);
    printf("ungrouped %lld\n", cocons::group_pairs_ungrouped(t));
    cocons::GroupPlan pl;
    const int status = cocons::group_plan(t, group.data(), pl);
    printf("status %d\n", status);
    if (status) return 0;
    printf("stats %d %d %d %lld %lld\n", pl.blocks, pl.maxrows, pl.longest, pl.sum_rows, pl.pairs);
    print("off", pl.off);
    print("rows", pl.rows);
    print("mask", pl.mask);
    print("order", pl.order);
    print("block", pl.block);
    print("pos", pl.pos);
    const int m_out = pl.longest > 1 ? pl.longest : 1;
    std::vector<int> out((size_t)n * m_out), byrow;
    cocons::group_table(pl, (size_t)n, m_out, out.data());
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m_out; ++j) byrow.push_back(out[(size_t)i + (size_t)j * n]);
    print("table", byrow);
    int have_k = 0, need_k = 0;
    const int bad = cocons::group_closed(t, pl, &have_k, &need_k);
    printf("closed %d %d %d\n", bad, have_k, need_k);
    // the expanded table is closed under the same partition, and its plan is the plan
    cocons::GroupTable e;
    e.p = out.data(); e.n = (size_t)n; e.m = m_out;
    cocons::GroupPlan pe;
    const int se = cocons::group_plan(e, group.data(), pe);
    printf("expanded %d %d %d\n", se, se ? -1 : cocons::group_closed(e, pe, nullptr, nullptr),
           se ? 0 : (int)(pe.rows == pl.rows && pe.off == pl.off && pe.mask == pl.mask));
    return 0;
}
