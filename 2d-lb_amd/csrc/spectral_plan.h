// spectral_plan.h -- the plan of the periodic 2-D FFT behind lb_spectral_* (kernels_spectral.h, spectral.cpp): which lengths are taken,
// the radix passes of an axis, how many rows / adjacent columns a workgroup transforms at once, the twiddle table.  Plain C++, no HIP
// (as plan.h): tests/spectral_plan_props.cpp links spectral_plan.cpp alone and sweeps every admissible length on a host.
//
// A workgroup holds its batch of 1-D transforms twice in LDS (Stockham autosort reads one copy and writes the other), 8 bytes an
// element: 2 x 8 x batch x n <= SP_LDS_BYTES.  That is what sets the longest axis: one transform of 4096 points fills the 64 KiB a
// workgroup may declare.  The column pass takes `cols` adjacent columns, so its global accesses are row segments of 8 x cols bytes:
// cols = min(nx, SP_MAX_BATCH_ELEMS / ny, 32, nx / SP_MIN_BLOCKS) and at least 1: by LDS 32 at ny <= 128, 16 at 256, ... 1 at ny > 2048, and
// never so wide that fewer than SP_MIN_BLOCKS workgroups -- one per CU -- are left where the box has that many columns (at 256^2
// blocks of 16 columns were 16 workgroups on 256 CUs); the rows likewise.
#pragma once

constexpr int SP_MAX_N = 4096;              // longest axis
constexpr int SP_MAX_PASSES = 12;           // (4096 = 2^12; with the radix-4 pass no admissible length needs more than 8)
constexpr int SP_LDS_BYTES = 65536;         // the LDS a workgroup of the transform kernels may ask for
constexpr int SP_THREADS = 256;
constexpr int SP_MAX_BATCH_ELEMS = SP_LDS_BYTES / 16;    // complex elements of one LDS copy
constexpr int SP_ROW_TARGET_ELEMS = 1024;   // rows: as many as make about four elements per thread
constexpr int SP_MAX_COLS = 32;             // columns: 256-byte row segments at most
constexpr int SP_MIN_BLOCKS = 256;          // workgroups a pass is cut into where the box allows it

struct SpAxis {
    int n;
    int npass;
    int radix[SP_MAX_PASSES];               // 5s, 3s, 4s, then a 2; their product is n
};

struct SpPlan {
    SpAxis x, y;
    int rows, row_blocks;                   // a workgroup of the row pass takes `rows` whole rows; ceil(ny / rows) workgroups
    int cols, col_blocks;                   // ... of the column pass `cols` adjacent columns; ceil(nx / cols) workgroups
    int row_lds_bytes, col_lds_bytes;
};

// n = 2^a 3^b 5^c, 1 <= n <= SP_MAX_N
bool sp_admissible(int n);
extern const char *const sp_length_rule;    // the sentence a refusal carries
// false: a length is not admissible (nothing is written)
bool sp_plan(int nx, int ny, SpPlan *out);
// exp(-2 pi i k / n), k < n, computed in double and rounded once: re_im[2k], re_im[2k + 1]
void sp_twiddles(int n, float *re_im);
// the integer wave index of element i of an axis of n points, as numpy's fftfreq orders them: 0 ... ceil(n/2) - 1, then -floor(n/2) ... -1
// (even n: the Nyquist index is -n/2)
constexpr int sp_wave_index(int i, int n) { return i < (n + 1) / 2 ? i : i - n; }
