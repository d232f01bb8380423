// spectral_plan_props.cpp -- the plan of the spectral solver's transform (2d-lb_amd/csrc/spectral_plan.cpp) on a host: its own main,
// spectral_plan.h, linked with spectral_plan.cpp only (tests/test_spectral_cpu.py builds it plain and under the sanitizers).
// For every pair of admissible axis lengths <= 4096 (`--thin`: every third pair):
//   S1_admissible      sp_admissible(n) is "n = 2^a 3^b 5^c, 1 <= n <= 4096" by trial division, for -3 <= n <= 5000; sp_plan refuses a
//                      pair with an inadmissible length and leaves its output alone
//   S2_radix_product   each axis: 0 <= npass <= SP_MAX_PASSES, every radix 2, 3, 4 or 5 (four bits hold it), the product is n
//   S3_lds             rows, cols >= 1; 16 x rows x nx and 16 x cols x ny are what the plan says and <= SP_LDS_BYTES
//   S4_coverage        the row blocks cover every row once, the column blocks every column once, no block is empty
//   S5_twiddles        per admissible length: entry 0 is (1, 0), every entry within 6e-8 of exp(-2 pi i k / n) in double, inside the table
// `--plan nx ny [nx ny ...]`: no sweep; one line per pair, "PLAN nx ny rows R cols C row_lds L col_lds L x r,r,... y r,r,..." ("-" for
// an axis without a pass), so that a test can hold the shapes it lists to the plan the library makes of them.
#include "spectral_plan.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

struct Prop {
    const char *name;
    long long cases = 0, bad = 0;
    void check(bool ok) { ++cases; if (!ok) ++bad; }
};

static bool smooth(int n)
{
    if (n < 1 || n > 4096) return false;
    for (int p = 2; p <= 5; ++p)
        while (p != 4 && n % p == 0) n /= p;
    return n == 1;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--plan")) {
        if (argc < 4 || argc % 2) return 2;
        for (int i = 2; i + 1 < argc; i += 2) {
            int nx = 0, ny = 0;
            SpPlan p;
            if (sscanf(argv[i], "%d", &nx) != 1 || sscanf(argv[i + 1], "%d", &ny) != 1 || !sp_plan(nx, ny, &p)) return 2;
            printf("PLAN %d %d rows %d cols %d row_lds %d col_lds %d", nx, ny, p.rows, p.cols, p.row_lds_bytes, p.col_lds_bytes);
            for (const SpAxis *a : {&p.x, &p.y}) {
                printf(a == &p.x ? " x " : " y ");
                if (!a->npass) printf("-");
                for (int k = 0; k < a->npass; ++k) printf(k ? ",%d" : "%d", a->radix[k]);
            }
            printf("\n");
        }
        return 0;
    }
    const bool thin = argc > 1 && !strcmp(argv[1], "--thin");
    Prop s1{"S1_admissible"}, s2{"S2_radix_product"}, s3{"S3_lds"}, s4{"S4_coverage"}, s5{"S5_twiddles"};
    std::vector<int> lens;
    for (int n = -3; n <= 5000; ++n) {
        s1.check(sp_admissible(n) == smooth(n));
        if (smooth(n)) lens.push_back(n);
    }
    for (int bad : {0, 7, 11, 14, 4097, 4100, 8192, -1}) {
        SpPlan p;
        memset(&p, 0x5a, sizeof p);
        const SpPlan before = p;
        s1.check(!sp_plan(bad, 8, &p) && !sp_plan(8, bad, &p) && !memcmp(&p, &before, sizeof p));
    }
    long long pair = 0;
    for (int nx : lens)
        for (int ny : lens) {
            if (thin && pair++ % 3) continue;
            SpPlan p;
            if (!sp_plan(nx, ny, &p)) { s1.check(false); continue; }
            for (const SpAxis *a : {&p.x, &p.y}) {
                long long prod = 1;
                bool ok = a->npass >= 0 && a->npass <= SP_MAX_PASSES && a->n == (a == &p.x ? nx : ny);
                for (int i = 0; ok && i < a->npass; ++i) {
                    ok = a->radix[i] >= 2 && a->radix[i] <= 5;
                    prod *= a->radix[i];
                }
                s2.check(ok && prod == a->n);
            }
            s3.check(p.rows >= 1 && p.cols >= 1 && p.row_lds_bytes == 16 * p.rows * nx && p.col_lds_bytes == 16 * p.cols * ny &&
                     p.row_lds_bytes <= SP_LDS_BYTES && p.col_lds_bytes <= SP_LDS_BYTES);
            // block b takes [b x per, min((b + 1) x per, n))
            for (int axis = 0; axis < 2; ++axis) {
                const int n = axis ? nx : ny, per = axis ? p.cols : p.rows, blocks = axis ? p.col_blocks : p.row_blocks;
                std::vector<int> seen((size_t)n, 0);
                bool ok = per >= 1 && blocks >= 1;
                for (int b = 0; ok && b < blocks; ++b) {
                    int taken = 0;
                    for (int i = b * per; i < (b + 1) * per && i < n; ++i) { ++seen[(size_t)i]; ++taken; }
                    ok = taken > 0;
                }
                for (int i = 0; ok && i < n; ++i) ok = seen[(size_t)i] == 1;
                s4.check(ok);
            }
        }
    for (int n : lens) {
        std::vector<float> t(2 * (size_t)n);
        sp_twiddles(n, t.data());
        bool ok = t[0] == 1.f && t[1] == 0.f;
        for (int k = 0; ok && k < n; ++k) {
            const double a = -2.0 * 3.14159265358979323846 * k / n;
            ok = fabs(t[2 * (size_t)k] - cos(a)) <= 6e-8 && fabs(t[2 * (size_t)k + 1] - sin(a)) <= 6e-8;
        }
        s5.check(ok);
    }
    int rc = 0;
    for (const Prop *p : {&s1, &s2, &s3, &s4, &s5}) {
        printf("%s cases=%lld bad=%lld\n", p->name, p->cases, p->bad);
        if (p->bad || !p->cases) rc = 1;
    }
    return rc;
}
