// The library's round rule (group_rounds of cocons_amd/csrc/group_plan.hpp) on the CPU, for
// tests/test_group_rounds_reference.py.  Input file: n, m, max_rows and max_rounds, then the n x m table row by row (1-based,
// 0 = none).  Output: one line per table, its name first: the labels, the rounds that merged something, group_plan's return
// on the labels and -- when that is 0 -- the plan's lines and the expanded table.
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
    int n = 0, m = 0, max_rows = 0, max_rounds = 0;
    if (fscanf(fh, "%d %d %d %d", &n, &m, &max_rows, &max_rounds) != 4 || n < 1 || m < 1 || max_rows < 2 || max_rows > 64 ||
        max_rounds < 0) {
        fprintf(stderr, "bad n, m, max_rows or max_rounds\n");
        return 2;
    }
    std::vector<int> nn((size_t)n * m), group((size_t)n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            int v = 0;
            if (fscanf(fh, "%d", &v) != 1 || v < 0 || v > i) { fprintf(stderr, "bad table entry in row %d\n", i + 1); return 2; }
            nn[(size_t)i + (size_t)j * n] = v;
        }
    fclose(fh);
    cocons::GroupTable t;
    t.p = nn.data(); t.n = (size_t)n; t.m = m;
    int rounds = -1;
    const int blocks = cocons::group_rounds(t, max_rows, max_rounds, group.data(), &rounds);
    print("group", group);
    printf("rounds %d\n", rounds);
    cocons::GroupPlan pl;
    const int status = cocons::group_plan(t, group.data(), pl);
    printf("status %d\n", status);
    if (status) return 0;
    printf("stats %d %d %d %lld %lld %d\n", pl.blocks, pl.maxrows, pl.longest, pl.sum_rows, pl.pairs, blocks);
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
    return 0;
}
