// kernels_poisson.h -- the kernels of the LB Poisson solver (LB_SEM_POISSON: the reference's LB_D2Q9/D2Q9_poisson.cl, driven as
// poisson/solver.py:324-358 does: rho_before = rho, move + copy_buffer -> move_bcs (nine times over) -> update_hydro -> update_feq ->
// collide_particles, six launches and six host waits per iteration, then two reductions and two host read-backs to decide whether to
// stop).  Included by poisson.cpp only (poisson_launch.h: what the kernels, their host code and the handle share; host.h: what the other host units see).
//   k_ps_step<RHO_ALWAYS>   the fused iteration on the lane-of-four plan (kernels_lane4.h): the gather without a wrap, the
//                           prescribed-density rule in registers on the lanes that hold a wall cell, one 16-byte load of the source.
//                           RHO_ALWAYS (lb_solve's form): the first instruction reads the stop word and the whole grid
//                           returns if it is set; the previous rho is loaded, the new one stored, and sum |rho_new - rho_old| and
//                           sum rho_old over the workgroup's cells inside the box go to its slot of the partials: 72 + 4 + 8 + 4 = 88 B
//                           per cell and iteration.  Otherwise (lb_run's form) no stop word, no sums, rho when the launch is the last.
//   k_ps_check              one workgroup: the partials in float64 in a fixed order, the ratio, the stop word
//   k_ps_gradient           central differences of rho into the handle's u, v planes (update_negative_gradient :256-306 without its
//                           sign and its swapped names)
//   k_ps_move_bcs, k_ps_hydro, k_ps_feq, k_ps_collide   the reference's phases one by one; scalar_cell.h's ps_* functions, the same
//                           operations as the fused cell: bitwise equal to it
// LB_BC_DIRICHLET, the reference's box: the gather is the one without a wrap (it reads row padding and ghost rows beside the box: inside
// the allocation, never used); on each wall and in each corner the three links pointing into the box become w_k R, R = -(sum of the
// cell's five other non-rest links + (w0 - 1) rho_on_boundary) / (sum of the three weights), every right-hand side a post-stream value
// of the same cell.  Two links per corner are neither streamed nor written and the corner's rule READS them: the handle's corner
// state, the same eight links in the same order as LB_BC_BOX's (row_wall, kernels_lane4.h).
#pragma once
#include "scalar_cell.h"
#include "poisson_launch.h"
#include "kernels_lane4.h"

namespace {

// move_bcs of D2Q9_poisson.cl:149-254 for one cell (w, e, s, n: it lies in column 0 / nx-1, row 0 / ny-1); st: the corner state;
// wall = (w0 - 1) rho_on_boundary.  The five links read are summed in ascending order, as every branch of the reference does (a
// written link contributes an exact + 0), and the three weights in ascending order of their links: 1/9 + 1/36 + 1/36 on a wall,
// 1/9 + 1/9 + 1/36 in a corner.
struct PsBox {
    float wall;
    __device__ __forceinline__ void rule(Cell &c, bool w, bool e, bool s, bool n, const float *st) const
    {
        if (s && w) { c.f6 = st[0]; c.f8 = st[1]; }
        if (s && e) { c.f5 = st[2]; c.f7 = st[3]; }
        if (n && w) { c.f5 = st[4]; c.f7 = st[5]; }
        if (n && e) { c.f6 = st[6]; c.f8 = st[7]; }
        // a link is written if it enters from outside -- except, in a corner, the two diagonals that run along the corner's other wall
        const bool wr[9] = {false, w, s, e, n, (w || s) && !(e || n), (e || s) && !(w || n), (e || n) && !(w || s), (w || n) && !(e || s)};
        const float f[9] = {0.f, c.f1, c.f2, c.f3, c.f4, c.f5, c.f6, c.f7, c.f8};
        float sum = 0.f;
#pragma unroll
        for (int k = 1; k < 9; ++k) sum = sum + (wr[k] ? 0.f : f[k]);
        const float w1 = 1.f / 9.f, w2 = 1.f / 36.f;
        const float den = ((w || e) && (s || n)) ? (w1 + w1) + w2 : (w1 + w2) + w2;
        const float R = -(sum + wall) / den;
        const float a1 = w1 * R, a2 = w2 * R;
        c.f1 = wr[1] ? a1 : c.f1;
        c.f2 = wr[2] ? a1 : c.f2;
        c.f3 = wr[3] ? a1 : c.f3;
        c.f4 = wr[4] ? a1 : c.f4;
        c.f5 = wr[5] ? a2 : c.f5;
        c.f6 = wr[6] ? a2 : c.f6;
        c.f7 = wr[7] ? a2 : c.f7;
        c.f8 = wr[8] ? a2 : c.f8;
    }
};

// moment, equilibrium, relaxation and source term of a lane's four gathered cells as two pairs (scalar_cell.h, T = f2a), in place
__device__ __forceinline__ void ps_collide_row(f4a (&q)[9], f4a s4, float omega, float react, f4a &r4)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f2a f[9], eq[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = pair_of(q[k], h);
        const f2a rho = ps_rho_t<f2a>(f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]);
        ps_feq_t<f2a>(eq, rho);
        ps_relax_t<f2a>(f, eq, omega, pair_of(s4, h) * lb_splat<f2a>(react));
        if (h) r4.zw = rho;
        else r4.xy = rho;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (h) q[k].zw = f[k];
            else q[k].xy = f[k];
        }
    }
}

// (lane_rows and the nine stores written out: every lane reaches the reduction, so there is no early return; through store_planes the plane offsets are shared with the gather's and the instruction text moves.)
// The two sums: a lane's four cells in order, the lanes of a wave through cross-lane moves, the four waves through LDS in index order;
// padding lanes, rows >= ny and columns >= nx are left out by selection, not by a factor (whatever the padding of rho holds).
template <bool RHO_ALWAYS>
__global__ __launch_bounds__(256) void k_ps_step(const StepArgs a, const PsExtra e)
{
    if (RHO_ALWAYS && e.state->stop != 0) return;       // (uniform over the grid: no kernel of this stream writes it meanwhile)
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int yl = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);
    float dsum = 0.f, rsum = 0.f;
    if (x4 < a.fpitch && yl < a.ny) {
        f4a q[9], r4;
        uc4 mk;
        gather_row<LB_BC_PIPE, false, false>(a, x4, yl, yl - 1, yl + 1, q, mk);     // (lane_gather written out: the call moves the diagnostic build's text)
        const long long m0 = (long long)yl * a.fpitch;
        const f4a s4 = load4<false>(lane_ptr(e.source + m0, x4));
        f4a o4 = {0.f, 0.f, 0.f, 0.f};
        if (RHO_ALWAYS) o4 = load4<false>(lane_ptr((const float *)a.rho + m0, x4));
        const int ce = a.nx - 1 - x4;
        if (yl == 0 || yl == a.ny - 1 || x4 == 0 || (ce >= 0 && ce < 4)) row_wall(PsBox{e.wall}, a.corner, a.nx, a.ny, x4, yl, q);
        ps_collide_row(q, s4, a.omega, e.react, r4);
        float *d = a.dst + (long long)yl * a.pitch;
        const long long S = a.plane;
#pragma unroll
        for (int k = 0; k < 9; ++k) store4<false>(lane_ptr(d + k * S, x4), q[k]);
        if (RHO_ALWAYS || e.store_rho) store4<false>(lane_ptr(a.rho + m0, x4), r4);
        if (RHO_ALWAYS) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = x4 + j < a.nx;
                dsum = dsum + (in ? fabsf(r4[j] - o4[j]) : 0.f);
                rsum = rsum + (in ? o4[j] : 0.f);
            }
        }
    }
    if (RHO_ALWAYS) {
        __shared__ float sh[2][4];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            dsum += __shfl_xor(dsum, m);
            rsum += __shfl_xor(rsum, m);
        }
        if (threadIdx.x == 0) { sh[0][threadIdx.y] = dsum; sh[1][threadIdx.y] = rsum; }
        __syncthreads();
        if (threadIdx.x == 0 && threadIdx.y == 0) {
            float *p = e.part + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
            p[0] = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
            p[1] = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
        }
    }
}

// One workgroup of 1024 threads: thread t sums the partials t, t + 1024, ... in float64 (four 8-byte loads in flight at a time), the
// lanes of a wave fold through cross-lane moves, the sixteen waves through LDS in index order: a fixed order, whatever order the
// workgroups of k_ps_step retired in.  The ratio mean |rho - rho_before| / mean rho_before (solver.py:350-354; the two weights
// 1 / (nx ny) cancel); iter >= 2 and ratio < tolerance -- false for the x/0 and 0/0 of a lattice that starts at zero -- sets the stop
// word.
constexpr int PS_CHECK_THREADS = 1024;
__global__ __launch_bounds__(PS_CHECK_THREADS) void k_ps_check(const float *part, long long n, PsState *state, int iter, float tolerance)
{
    if (state->stop != 0) return;                       // (an iteration behind the stop: its k_ps_step did nothing, the partials are stale)
    constexpr int WAVES = PS_CHECK_THREADS / 64;
    __shared__ double sh[2][WAVES];
    const float2 *p2 = reinterpret_cast<const float2 *>(part);
    double d = 0., r = 0.;
#pragma unroll 4
    for (long long i = threadIdx.x; i < n; i += PS_CHECK_THREADS) {
        const float2 p = p2[i];
        d += (double)p.x;
        r += (double)p.y;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        d += __shfl_xor(d, m);
        r += __shfl_xor(r, m);
    }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = d; sh[1][threadIdx.x >> 6] = r; }
    __syncthreads();
    if (threadIdx.x == 0) {
        d = sh[0][0];
        r = sh[1][0];
        for (int i = 1; i < WAVES; ++i) { d += sh[0][i]; r += sh[1][i]; }
        const double ratio = d / r;
        state->ratio = (float)ratio;
        state->ratio_iter = iter;
        if (iter >= 2 && ratio < (double)tolerance) state->stop = iter;
    }
}

// ---- one cell per thread: grid = (ceil(nx / 256), ny) ---------------------------------------------------------------------------------
__global__ void k_ps_gradient(const StepArgs a, float inv_two_dx)      // a.u := d rho / dx, a.v := d rho / dy
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long o = (long long)y * a.fpitch + x;
    const float *r = a.rho + o;
    const float xp = x + 1 < a.nx ? r[1] : 0.f, xm = x >= 1 ? r[-1] : 0.f;
    const float yp = y + 1 < a.ny ? r[a.fpitch] : 0.f, ym = y >= 1 ? r[-a.fpitch] : 0.f;
    a.u[o] = (xp - xm) * inv_two_dx;
    a.v[o] = (yp - ym) * inv_two_dx;
}

__global__ void k_ps_hydro(const StepArgs a)
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const float *f = a.src + (long long)y * a.pitch + x;
    const long long S = a.plane;
    a.rho[(long long)y * a.fpitch + x] = ps_rho_t<float>(f[S], f[2 * S], f[3 * S], f[4 * S], f[5 * S], f[6 * S], f[7 * S], f[8 * S]);
}

__global__ void k_ps_feq(const StepArgs a, float *feq)
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    float e[9];
    ps_feq_t<float>(e, a.rho[(long long)y * a.fpitch + x]);
    float *o = feq + (long long)y * a.pitch + x;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k * a.plane] = e[k];
}

// (cell_xy written out: the call moves the instruction text)
__global__ void k_ps_collide(const StepArgs a, float *f, const float *feq, const float *source, float react)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.nx) return;
    const long long o = (long long)y * a.pitch + x;
    float c[9], e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { c[k] = f[o + k * a.plane]; e[k] = feq[o + k * a.plane]; }
    ps_relax_t<float>(c, e, a.omega, source[(long long)y * a.fpitch + x] * react);
#pragma unroll
    for (int k = 0; k < 9; ++k) f[o + k * a.plane] = c[k];
}

// move_bcs of one lattice, in place behind lb_move (edge_walk, kernels_lane4.h).  The two links per corner that the rule reads but
// never writes are what the lattice holds (lb_move has patched the corner state in).
__global__ void k_ps_move_bcs(const StepArgs a, float *f, float wall) { edge_walk(a, f, BoxEdge<PsBox>{{wall}}); }

}  // namespace
