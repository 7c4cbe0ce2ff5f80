// The library's envelope rule and packed band layout (cocons_amd/csrc/band_plan.hpp) on the CPU, for
// tests/test_taper_envelope_cases.py.  Input file: n, then n + 1 row pointers and the column indices of a 1-based CSR in the
// handle's order; "0 nt" instead asks for the plan of a handle of nt tile columns without an envelope.  Output: one line per
// table, its name first.  With the one argument "buckets" it runs band_buckets on a pattern read from standard input instead:
// nt, n and inv[0 .. n) (the position of each of the caller's n columns), m and the m + 1 row pointers and column indices of a
// 1-based CSR of m rows, then row0, nrows and stride; it prints hci, hdst, hsrc and boff.
#include <cstring>
#include <cstdio>
#include <vector>

#include "band_plan.hpp"

static void print(const char *name, const std::vector<int> &v)
{
    printf("%s", name);
    for (int x : v) printf(" %d", x);
    printf("\n");
}

static int buckets_main()
{
    int nt = 0, n = 0, m = 0, row0 = 0, nrows = 0, stride = 0;
    if (scanf("%d %d", &nt, &n) != 2 || nt < 1 || n < 1) { fprintf(stderr, "bad nt or n\n"); return 2; }
    std::vector<int> inv((size_t)n);
    for (int &x : inv) if (scanf("%d", &x) != 1 || x < 0 || x >= nt * 128) { fprintf(stderr, "bad inv\n"); return 2; }
    if (scanf("%d", &m) != 1 || m < 1) { fprintf(stderr, "bad m\n"); return 2; }
    std::vector<int> rp((size_t)m + 1);
    for (int &x : rp) if (scanf("%d", &x) != 1) { fprintf(stderr, "short row pointers\n"); return 2; }
    if (rp[0] != 1) { fprintf(stderr, "not a 1-based CSR\n"); return 2; }
    for (int i = 0; i < m; ++i) if (rp[i + 1] < rp[i]) { fprintf(stderr, "row pointers decrease\n"); return 2; }
    std::vector<int> ci((size_t)rp[m] - 1);
    for (int &x : ci) if (scanf("%d", &x) != 1 || x < 1 || x > n) { fprintf(stderr, "bad column index\n"); return 2; }
    if (scanf("%d %d %d", &row0, &nrows, &stride) != 3 || row0 < 0 || nrows < 0 || row0 + nrows > m || stride < nrows) {
        fprintf(stderr, "bad row0, nrows or stride\n");
        return 2;
    }
    std::vector<int> hci, hdst, hsrc, boff;
    cocons::band_buckets<128>(nt, inv.data(), ci.data(), rp.data(), row0, nrows, stride, hci, hdst, hsrc, boff);
    print("hci", hci);
    print("hdst", hdst);
    print("hsrc", hsrc);
    print("boff", boff);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "buckets")) return buckets_main();
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n = 0, nt = 0;
    if (fscanf(fh, "%d", &n) != 1 || n < 0) { fprintf(stderr, "bad n\n"); return 2; }
    cocons::BandEnvelope env;
    if (n > 0) {
        std::vector<int> rp((size_t)n + 1);
        for (int &x : rp) if (fscanf(fh, "%d", &x) != 1) { fprintf(stderr, "short row pointers\n"); return 2; }
        if (rp[0] != 1) { fprintf(stderr, "not a 1-based CSR\n"); return 2; }
        for (int i = 0; i < n; ++i) if (rp[i + 1] < rp[i]) { fprintf(stderr, "row pointers decrease\n"); return 2; }
        std::vector<int> ci((size_t)rp[n] - 1);
        for (int &x : ci) if (fscanf(fh, "%d", &x) != 1 || x < 1 || x > n) { fprintf(stderr, "bad column index\n"); return 2; }
        env = cocons::band_envelope(n, rp.data(), ci.data(), 128);
        nt = (int)env.hi.size();
    } else if (fscanf(fh, "%d", &nt) != 1 || nt < 1) { fprintf(stderr, "bad nt\n"); return 2; }
    fclose(fh);
    cocons::BandPlan pl;
    const char *why = cocons::band_plan(nt, n > 0 ? env.hi.data() : nullptr, env.maxband, pl);
    printf("nt %d\nmaxband %d\nstatus %d\nW %d\n", nt, env.maxband, why ? 1 : 0, pl.W);
    if (why) fprintf(stderr, "%s\n", why);
    print("envelope", env.hi);
    print("hi", pl.hi);
    print("hib", pl.hib);
    print("toff", pl.toff);
    print("toffb", pl.toffb);
    return 0;
}
