// kernels_spectral.h -- the periodic 2-D FFT that solves (1 - lambda^2 lap) phi = rho and returns grad phi (the reference's
// spectral_poisson/screened_poisson.py: three gpyfft plans and a dozen whole-array passes per solve, a host wait behind each).
// Included by spectral.cpp only.  Complex float32, interleaved, [ny][nx]; the plan is spectral_plan.h's.
//   k_sp_rows_fwd<REAL>   the x-FFT of whole rows, in place in a dense complex array -- or (REAL) from a real plane at a lattice's pitch
//   k_sp_cols_mid         a block of adjacent columns: forward y-FFT, the screening 1 / (lambda^2 (kx^2 + ky^2) + 1) on the way out
//                         to `charge`, then for each gradient the multiplier 2 pi i k on the way in and an inverse y-FFT -- three
//                         transforms in LDS, nothing transposed in global memory
//   k_sp_rows_inv<VEL>    the inverse x-FFT of both gradients (blockIdx.y) and 1 / (nx ny); VEL: the real part times `scale` straight
//                         into u and v of a lattice, cells x < nx only
//   k_sp_cols<INV>, k_sp_screen, k_sp_grad   the phases one by one (lb_spectral_transform, _screen, _grad_multiply)
// The transform: Stockham autosort, decimation in frequency, radix 5 / 3 / 4 / 2 passes between two LDS copies of the workgroup's batch
// (sp_pass); element j of transform b lives at b n + j (rows) or j B + b (columns: a thread's neighbours are the block's other
// columns, so LDS and global accesses are both contiguous).  The inverse is the forward transform of the data with real and imaginary
// parts exchanged on the way in and on the way out.  Twiddles come from a table the host computed in double (sp_twiddles); every
// multiply-add is an explicit lb_fma and every other statement one operation, so the fused kernels and the phases -- the same device
// functions -- give the same bits.
#pragma once
#include "d2q9_cell.h"          // lb_fma
#include "spectral_plan.h"

namespace {

typedef float2 cf;

struct SpDevAxis {
    int n, npass;
    unsigned long long radices;     // four bits a pass, first pass lowest
};

struct SpArgs {
    cf *c, *x, *y;                  // the array a single transform works on / charge; xgrad; ygrad
    const cf *twx, *twy;            // exp(-2 pi i k / n) of each axis
    const float *real_in;           // k_sp_rows_fwd<true>: [ny][rpitch]
    float *u, *v;                   // k_sp_rows_inv<true>: [ny][rpitch]
    int rpitch;
    int nx, ny;
    int rows, cols;                 // SpPlan
    float lam2, norm, scale;        // lambda^2; 1 / (nx ny); the velocity's factor
    SpDevAxis ax, ay;
};

__device__ __forceinline__ cf c_make(float x, float y) { cf r; r.x = x; r.y = y; return r; }
__device__ __forceinline__ cf c_add(cf a, cf b) { return c_make(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cf c_sub(cf a, cf b) { return c_make(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cf c_swap(cf a) { return c_make(a.y, a.x); }
__device__ __forceinline__ cf c_mul(cf a, cf w)
{
    const float pr = a.x * w.x, pi = a.x * w.y;
    return c_make(lb_fma(-a.y, w.y, pr), lb_fma(a.y, w.x, pi));
}
// a + (-i) b and a + i b
__device__ __forceinline__ cf c_add_mi(cf a, cf b) { return c_make(a.x + b.y, a.y - b.x); }
__device__ __forceinline__ cf c_add_pi(cf a, cf b) { return c_make(a.x - b.y, a.y + b.x); }

// value / (lambda^2 (kx^2 + ky^2) + 1): the integer kx^2 + ky^2 <= 2 x 2048^2 is exact in float32
__device__ __forceinline__ cf sp_screen(cf v, int kx, int ky, float lam2)
{
    const float kk = (float)(kx * kx + ky * ky);
    const float den = lb_fma(lam2, kk, 1.f);
    const float r = 1.f / den;
    return c_make(v.x * r, v.y * r);
}

// value x 2 pi i k
__device__ __forceinline__ cf sp_gradmul(cf v, int k)
{
    const float g = 6.2831853071795864769f * (float)k;
    const float re = g * v.y, im = g * v.x;
    return c_make(-re, im);
}

// Every butterfly gives (r a, 0, ..., 0) EXACTLY on r equal inputs a, and the plan takes the odd radices first: a constant row and the
// Nyquist mode (-1)^x -- whose gradient the reference keeps an imaginary part of -- then transform without a rounding error, as they do
// in pocketfft; with the factor 2 first or the textbook radix 5 (a0 + c1 s14 + c2 s23) the zeros of the Nyquist row come out as
// 1e-7 of its peak, and the screening, which divides the peak by 1 + n^2 / 4, makes that 1e-6 ... 1e-4 of the screened spectrum.
// One radix-r pass over the batch: butterfly t = p s + q of transform b reads src[q + s p + k m], k < r, m = n / r, and writes
// dst[q + s (r p + j)] = (DFT_r a)_j x exp(-2 pi i p s j / n).
template <bool COLS>
__device__ __forceinline__ void sp_pass(const cf *src, cf *dst, const cf *tw, int n, int B, int r, int s)
{
    const int m = n / r, total = B * m;
    const int sj = COLS ? B : 1;
    for (int idx = threadIdx.x; idx < total; idx += SP_THREADS) {
        int b, t;
        if (COLS) { t = idx / B; b = idx - t * B; }
        else { b = idx / m; t = idx - b * m; }
        const int p = t / s, q = t - p * s;
        const int base = COLS ? b : b * n;
        const cf *in = src + base + (q + s * p) * sj;
        cf *out = dst + base + (q + s * r * p) * sj;
        const int is = m * sj, os = s * sj, ws = p * s;
        if (r == 4) {
            const cf a0 = in[0], a1 = in[is], a2 = in[2 * is], a3 = in[3 * is];
            const cf s02 = c_add(a0, a2), d02 = c_sub(a0, a2), s13 = c_add(a1, a3), d13 = c_sub(a1, a3);
            out[0] = c_add(s02, s13);
            out[os] = c_mul(c_add_mi(d02, d13), tw[ws]);
            out[2 * os] = c_mul(c_sub(s02, s13), tw[2 * ws]);
            out[3 * os] = c_mul(c_add_pi(d02, d13), tw[3 * ws]);
        } else if (r == 2) {
            const cf a0 = in[0], a1 = in[is];
            out[0] = c_add(a0, a1);
            out[os] = c_mul(c_sub(a0, a1), tw[ws]);
        } else if (r == 3) {
            const float h = 0.86602540378443864676f;        // sin(2 pi / 3)
            const cf a0 = in[0], a1 = in[is], a2 = in[2 * is];
            const cf sm = c_add(a1, a2), d = c_sub(a1, a2);
            const cf tt = c_make(lb_fma(-0.5f, sm.x, a0.x), lb_fma(-0.5f, sm.y, a0.y));
            const cf hd = c_make(h * d.x, h * d.y);
            out[0] = c_add(a0, sm);
            out[os] = c_mul(c_add_mi(tt, hd), tw[ws]);
            out[2 * os] = c_mul(c_add_pi(tt, hd), tw[2 * ws]);
        } else {
            const float c1 = 0.30901699437494742410f;                                   // cos(2 pi / 5); cos(4 pi / 5) = -1/2 - c1
            const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;     // sin(2 pi / 5), sin(4 pi / 5)
            const cf a0 = in[0], a1 = in[is], a2 = in[2 * is], a3 = in[3 * is], a4 = in[4 * is];
            const cf s14 = c_add(a1, a4), d14 = c_sub(a1, a4), s23 = c_add(a2, a3), d23 = c_sub(a2, a3);
            // a0 + c1 s14 + c2 s23 with c2 = -1/2 - c1: exactly zero on equal inputs, like every other butterfly here (below)
            const cf dd = c_sub(s14, s23);
            const cf t1 = c_make(lb_fma(c1, dd.x, lb_fma(-0.5f, s23.x, a0.x)), lb_fma(c1, dd.y, lb_fma(-0.5f, s23.y, a0.y)));
            const cf t2 = c_make(lb_fma(-c1, dd.x, lb_fma(-0.5f, s14.x, a0.x)), lb_fma(-c1, dd.y, lb_fma(-0.5f, s14.y, a0.y)));
            const float p1x = s1 * d14.x, p1y = s1 * d14.y, p2x = s2 * d14.x, p2y = s2 * d14.y;
            const cf u1 = c_make(lb_fma(s2, d23.x, p1x), lb_fma(s2, d23.y, p1y));
            const cf u2 = c_make(lb_fma(-s1, d23.x, p2x), lb_fma(-s1, d23.y, p2y));
            out[0] = c_add(a0, c_add(s14, s23));
            out[os] = c_mul(c_add_mi(t1, u1), tw[ws]);
            out[2 * os] = c_mul(c_add_mi(t2, u2), tw[2 * ws]);
            out[3 * os] = c_mul(c_add_pi(t2, u2), tw[3 * ws]);
            out[4 * os] = c_mul(c_add_pi(t1, u1), tw[4 * ws]);
        }
    }
}

// the batch in LDS copy a, forward-transformed; returns the copy that holds the result, every thread past the last barrier
template <bool COLS>
__device__ __forceinline__ cf *sp_fft(cf *a, cf *b, const SpDevAxis &ax, int B, const cf *tw)
{
    int s = 1;
    for (int i = 0; i < ax.npass; ++i) {
        const int r = (int)((ax.radices >> (4 * i)) & 15u);
        __syncthreads();
        sp_pass<COLS>(a, b, tw, ax.n, B, r, s);
        s *= r;
        cf *t = a; a = b; b = t;
    }
    __syncthreads();
    return a;
}

// every element e of the workgroup's batch, the thread's own each time: f(e, x, y, inside the array)
template <bool COLS, typename F>
__device__ __forceinline__ void sp_each(int n, int B, int b0, int limit, F f)
{
    for (int e = threadIdx.x; e < B * n; e += SP_THREADS) {
        int b, j;
        if (COLS) { j = e / B; b = e - j * B; }
        else { b = e / n; j = e - b * n; }
        f(e, COLS ? b0 + b : j, COLS ? j : b0 + b, b0 + b < limit);
    }
}

extern __shared__ cf sp_lds[];

template <bool REAL>
__global__ __launch_bounds__(SP_THREADS) void k_sp_rows_fwd(const SpArgs a)
{
    const int n = a.nx, B = a.rows, b0 = blockIdx.x * B;
    cf *l0 = sp_lds, *l1 = sp_lds + B * n;
    sp_each<false>(n, B, b0, a.ny, [&](int e, int x, int y, bool in) {
        cf v = c_make(0.f, 0.f);
        if (in) {
            if (REAL) v.x = a.real_in[(long long)y * a.rpitch + x];
            else v = a.c[(long long)y * n + x];
        }
        l0[e] = v;
    });
    const cf *res = sp_fft<false>(l0, l1, a.ax, B, a.twx);
    sp_each<false>(n, B, b0, a.ny, [&](int e, int x, int y, bool in) {
        if (in) a.c[(long long)y * n + x] = res[e];
    });
}

template <bool VEL>
__global__ __launch_bounds__(SP_THREADS) void k_sp_rows_inv(const SpArgs a)
{
    const int n = a.nx, B = a.rows, b0 = blockIdx.x * B;
    cf *l0 = sp_lds, *l1 = sp_lds + B * n;
    cf *g = blockIdx.y ? a.y : a.x;
    float *w = blockIdx.y ? a.v : a.u;
    sp_each<false>(n, B, b0, a.ny, [&](int e, int x, int y, bool in) {
        l0[e] = in ? c_swap(g[(long long)y * n + x]) : c_make(0.f, 0.f);
    });
    const cf *res = sp_fft<false>(l0, l1, a.ax, B, a.twx);
    sp_each<false>(n, B, b0, a.ny, [&](int e, int x, int y, bool in) {
        if (!in) return;
        const cf r = c_swap(res[e]);
        const float re = r.x * a.norm, im = r.y * a.norm;
        if (VEL) w[(long long)y * a.rpitch + x] = re * a.scale;
        else g[(long long)y * n + x] = c_make(re, im);
    });
}

template <bool INV>
__global__ __launch_bounds__(SP_THREADS) void k_sp_cols(const SpArgs a)
{
    const int n = a.ny, B = a.cols, b0 = blockIdx.x * B;
    cf *l0 = sp_lds, *l1 = sp_lds + B * n;
    sp_each<true>(n, B, b0, a.nx, [&](int e, int x, int y, bool in) {
        const cf v = in ? a.c[(long long)y * a.nx + x] : c_make(0.f, 0.f);
        l0[e] = INV ? c_swap(v) : v;
    });
    const cf *res = sp_fft<true>(l0, l1, a.ay, B, a.twy);
    sp_each<true>(n, B, b0, a.nx, [&](int e, int x, int y, bool in) {
        if (in) a.c[(long long)y * a.nx + x] = INV ? c_swap(res[e]) : res[e];
    });
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_cols_mid(const SpArgs a)
{
    const int n = a.ny, B = a.cols, b0 = blockIdx.x * B;
    cf *l0 = sp_lds, *l1 = sp_lds + B * n;
    sp_each<true>(n, B, b0, a.nx, [&](int e, int x, int y, bool in) {
        l0[e] = in ? a.c[(long long)y * a.nx + x] : c_make(0.f, 0.f);
    });
    const cf *res = sp_fft<true>(l0, l1, a.ay, B, a.twy);
    sp_each<true>(n, B, b0, a.nx, [&](int e, int x, int y, bool in) {
        if (in) a.c[(long long)y * a.nx + x] = sp_screen(res[e], sp_wave_index(x, a.nx), sp_wave_index(y, n), a.lam2);
    });
    // (a thread reads back the elements it stored itself, and writes the LDS slots it has just read or ones nobody reads before the
    // next barrier)
    for (int which = 0; which < 2; ++which) {
        cf *g = which ? a.y : a.x;
        sp_each<true>(n, B, b0, a.nx, [&](int e, int x, int y, bool in) {
            cf v = c_make(0.f, 0.f);
            if (in) v = sp_gradmul(a.c[(long long)y * a.nx + x], which ? sp_wave_index(y, n) : sp_wave_index(x, a.nx));
            l0[e] = c_swap(v);
        });
        res = sp_fft<true>(l0, l1, a.ay, B, a.twy);
        sp_each<true>(n, B, b0, a.nx, [&](int e, int x, int y, bool in) {
            if (in) g[(long long)y * a.nx + x] = c_swap(res[e]);
        });
    }
}

// ---- the phases that are not transforms: one element per thread, grid = ceil(nx ny / 256) ---------------------------------------------
__global__ __launch_bounds__(SP_THREADS) void k_sp_screen(const SpArgs a)
{
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= a.nx * a.ny) return;
    const int y = i / a.nx, x = i - y * a.nx;
    a.c[i] = sp_screen(a.c[i], sp_wave_index(x, a.nx), sp_wave_index(y, a.ny), a.lam2);
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_grad(const SpArgs a)
{
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= a.nx * a.ny) return;
    const int y = i / a.nx, x = i - y * a.nx;
    const cf v = a.c[i];
    a.x[i] = sp_gradmul(v, sp_wave_index(x, a.nx));
    a.y[i] = sp_gradmul(v, sp_wave_index(y, a.ny));
}

}  // namespace
