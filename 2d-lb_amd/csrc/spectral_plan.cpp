// spectral_plan.cpp -- spectral_plan.h's arithmetic.  No HIP.
#include "spectral_plan.h"

#include <math.h>

#include <initializer_list>

const char *const sp_length_rule = "an axis of the spectral solver has 1 ... 4096 points and no prime factor other than 2, 3 and 5 (n = 2^a 3^b 5^c)";

bool sp_admissible(int n)
{
    if (n < 1 || n > SP_MAX_N) return false;
    for (int p : {2, 3, 5})
        while (n % p == 0) n /= p;
    return n == 1;
}

static void plan_axis(int n, SpAxis *a)
{
    a->n = n;
    a->npass = 0;
    for (int i = 0; i < SP_MAX_PASSES; ++i) a->radix[i] = 1;
    for (int r : {5, 3, 4, 2})       // (odd radices first: kernels_spectral.h has why)
        while (n % r == 0) {
            a->radix[a->npass++] = r;
            n /= r;
        }
}

static int min3(int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }

bool sp_plan(int nx, int ny, SpPlan *out)
{
    if (!sp_admissible(nx) || !sp_admissible(ny)) return false;
    SpPlan p;
    plan_axis(nx, &p.x);
    plan_axis(ny, &p.y);
    p.rows = min3(ny, SP_ROW_TARGET_ELEMS / nx, SP_MAX_BATCH_ELEMS / nx);
    if (p.rows > ny / SP_MIN_BLOCKS) p.rows = ny / SP_MIN_BLOCKS;     // (a small box: rather a workgroup on every CU than full batches on a few)
    if (p.rows < 1) p.rows = 1;
    p.row_blocks = (ny + p.rows - 1) / p.rows;
    p.cols = min3(nx, SP_MAX_BATCH_ELEMS / ny, SP_MAX_COLS);
    if (p.cols > nx / SP_MIN_BLOCKS) p.cols = nx / SP_MIN_BLOCKS;
    if (p.cols < 1) p.cols = 1;
    p.col_blocks = (nx + p.cols - 1) / p.cols;
    p.row_lds_bytes = 16 * p.rows * nx;
    p.col_lds_bytes = 16 * p.cols * ny;
    *out = p;
    return true;
}

void sp_twiddles(int n, float *re_im)
{
    const double step = -2.0 * 3.14159265358979323846 / (double)n;
    for (int k = 0; k < n; ++k) {
        // (the quarter points exactly: cos and sin of a rounded multiple of pi leave 6e-17 where 0 belongs)
        double c = cos(step * k), s = sin(step * k);
        if (4 * k == n) { c = 0.0; s = -1.0; }
        if (2 * k == n) { c = -1.0; s = 0.0; }
        if (4 * k == 3 * n) { c = 0.0; s = 1.0; }
        re_im[2 * k] = (float)c;
        re_im[2 * k + 1] = (float)s;
    }
}
