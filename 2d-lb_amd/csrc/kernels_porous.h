// kernels_porous.h -- the kernels of forced flow in a porous medium (LB_SEM_POROUS: the reference's
// LB_D2Q9/porous_media/single_component.cl, driven as single_component.py:679-751 does with one fluid: move[_periodic] ->
// copy_streamed_onto_f -> move_open_bcs -> update_hydro_pourous -> Gx, Gy = 0 -> the additional forces -> update_forces_pourous ->
// update_bary_velocity -> update_feq_pourous -> collide_particles_pourous, eleven launches and eleven host waits per step).  Included
// by porous.cpp only (porous_launch.h: what the kernels and their host code share; host.h: what the other host units see).
//   k_pm_step<BC, FIELD, LAST>   the fused step on k_ad_step's plan (kernels_scalar.h): a lane owns four consecutive cells of a row; nine
//                                16-byte loads (six displaced by one element: k_step's gather), FIELD: two 16-byte loads of the
//                                force field, the eight stages in registers (porous_cell.h), nine aligned 16-byte stores; LAST (a
//                                run's last launch): seven more of rho, u, v, Gx, Gy, u_b, v_b.  72 B per cell and step, 80 B with a
//                                field, + 28 B on the last.
//   k_pm_move_bcs, k_pm_hydro, k_pm_forces, k_pm_bary, k_pm_feq, k_pm_collide   the reference's phases one by one; porous_cell.h's
//                                functions, the same operations as the fused cell: bitwise equal to it
// LB_BC_PERIODIC: the gather wraps as k_ad_step's does.  LB_BC_ZERO_GRADIENT: cell (x, y) is, after move + move_open_bcs, a copy of the
// post-stream interior cell (xs, ys) = (clamp(x, 1, nx-2), clamp(y, 1, ny-2)), so in pull form it gathers link k from
// (xs - c_kx, ys - c_ky): the SOURCE cell is clamped.  In y the clamp is wave-uniform -- rows 0 and ny-1 simply gather what rows 1 and
// ny-2 gather, no second load; in x the cell x = 0 takes the gathered cell x = 1 of its own lane, the cell x = nx-1 the gathered cell
// nx-2: a select where that is in the lane, nine scalar loads on that one lane where nx-1 is a lane's first cell.  The gather itself is
// the one without a wrap (it reads row padding beside the box: inside the allocation, replaced by the selects).
#pragma once
#include "porous_cell.h"

namespace {

// ZERO_GRADIENT, x: the lane's cells x = 0 and x = nx-1 become copies of their interior neighbours (ys: the clamped row)
__device__ __forceinline__ void pm_clamp_x(const StepArgs &a, int x4, int ys, f4a (&q)[9])
{
    if (x4 == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) q[k].x = q[k].y;
    }
    const int c = a.nx - 1 - x4;
    if (c == 0) {
        // the neighbour is the last cell of the lane before: gathered again, link k from (nx-2 - c_kx, ys - c_ky)
        const long long P = a.pitch, S = a.plane;
        const float *r0 = a.src + (long long)ys * P + (a.nx - 2), *rm = r0 - P, *rp = r0 + P;
        q[0].x = r0[0];
        q[1].x = r0[1 * S - 1];
        q[2].x = rm[2 * S];
        q[3].x = r0[3 * S + 1];
        q[4].x = rp[4 * S];
        q[5].x = rm[5 * S - 1];
        q[6].x = rm[6 * S + 1];
        q[7].x = rp[7 * S + 1];
        q[8].x = rp[8 * S - 1];
    } else if (c > 0 && c < 4) {
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int j = 1; j < 4; ++j) q[k][j] = j == c ? q[k][j - 1] : q[k][j];
    }
}

// stages 3-8 of a lane's four gathered cells as two pairs (porous_cell.h, T = f2a), in place; g4x, g4y: the body force of the cells
__device__ __forceinline__ void pm_collide_row(const PmExtra &e, float omega, f4a (&q)[9], f4a g4x, f4a g4y, f4a &r4, f4a &u4,
                                               f4a &v4, f4a &Gx4, f4a &Gy4, f4a &ub4, f4a &vb4)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f2a f[9], eq[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = h ? q[k].zw : q[k].xy;
        f2a rho, mx, my, u, v;
        pm_hydro_t<f2a>(f, rho, mx, my, u, v);
        const f2a mag = pm_speed_t<f2a>(u, v);
        const f2a Gx = pm_force_t<f2a>(e, rho, h ? g4x.zw : g4x.xy, u, mag);
        const f2a Gy = pm_force_t<f2a>(e, rho, h ? g4y.zw : g4y.xy, v, mag);
        const f2a ub = pm_bary_t<f2a>(rho, mx, Gx);
        const f2a vb = pm_bary_t<f2a>(rho, my, Gy);
        pm_feq_t<f2a>(e, eq, rho, ub, vb);
        pm_relax_t<f2a>(e, f, eq, omega, rho, ub, vb, Gx, Gy);
        if (h) { r4.zw = rho; u4.zw = u; v4.zw = v; Gx4.zw = Gx; Gy4.zw = Gy; ub4.zw = ub; vb4.zw = vb; }
        else { r4.xy = rho; u4.xy = u; v4.xy = v; Gx4.xy = Gx; Gy4.xy = Gy; ub4.xy = ub; vb4.xy = vb; }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (h) q[k].zw = f[k];
            else q[k].xy = f[k];
        }
    }
}

// Launch: blockDim = (64, 4), grid = (ceil(fpitch / 256), ceil(ny / 4)): a wave covers 256 cells of one row (k_ad_step's launch).
template <int BC, bool FIELD, bool LAST>
__global__ __launch_bounds__(256) void k_pm_step(const StepArgs a, const PmExtra e)
{
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int yl = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);
    if (x4 >= a.fpitch || yl >= a.ny) return;
    int ys = yl;                            // the row of the source cells
    if (BC == LB_BC_ZERO_GRADIENT) ys = min(max(yl, 1), a.ny - 2);
    int ym = ys - 1, yp = ys + 1;           // source rows of the cy = +1 / cy = -1 links
    if (BC == LB_BC_PERIODIC) {
        if (ym < 0) ym = a.ny - 1;
        if (yp >= a.ny) yp = 0;
    }
    f4a q[9];
    uc4 mk;
    gather_row<BC == LB_BC_PERIODIC ? LB_BC_PERIODIC : LB_BC_PIPE, false, false>(a, x4, ys, ym, yp, q, mk);
    const long long m0 = (long long)yl * a.fpitch;
    f4a g4x = {e.gx, e.gx, e.gx, e.gx}, g4y = {e.gy, e.gy, e.gy, e.gy};
    if (FIELD) {
        g4x = g4x + load4<false>(lane_ptr(e.fgx + m0, x4));
        g4y = g4y + load4<false>(lane_ptr(e.fgy + m0, x4));
    }
    if (BC == LB_BC_ZERO_GRADIENT) pm_clamp_x(a, x4, ys, q);
    f4a r4, u4, v4, Gx4, Gy4, ub4, vb4;
    pm_collide_row(e, a.omega, q, g4x, g4y, r4, u4, v4, Gx4, Gy4, ub4, vb4);
    float *d = a.dst + (long long)yl * a.pitch;
    const long long S = a.plane;
#pragma unroll
    for (int k = 0; k < 9; ++k) store4<false>(lane_ptr(d + k * S, x4), q[k]);
    if (LAST) {
        store_moments(a, m0, x4, r4, u4, v4);
        store4<false>(lane_ptr(e.Gx + m0, x4), Gx4);
        store4<false>(lane_ptr(e.Gy + m0, x4), Gy4);
        store4<false>(lane_ptr(e.ub + m0, x4), ub4);
        store4<false>(lane_ptr(e.vb + m0, x4), vb4);
    }
}

// ---- the reference's phases, one cell per thread: grid = (ceil(nx / 256), ny) ---------------------------------------------------
__device__ __forceinline__ void pm_load_cell(const float *p, long long S, float (&f)[9])
{
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = p[k * S];
}

__global__ void k_pm_hydro(const StepArgs a)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.nx) return;
    float f[9], rho, mx, my, u, v;
    pm_load_cell(a.src + (long long)y * a.pitch + x, a.plane, f);
    pm_hydro_t<float>(f, rho, mx, my, u, v);
    const long long m = (long long)y * a.fpitch + x;
    a.rho[m] = rho; a.u[m] = u; a.v[m] = v;
}

__global__ void k_pm_forces(const StepArgs a, const PmExtra e)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.nx) return;
    const long long m = (long long)y * a.fpitch + x;
    float gx = e.gx, gy = e.gy;
    if (e.fgx) { gx = gx + e.fgx[m]; gy = gy + e.fgy[m]; }
    const float rho = a.rho[m], u = a.u[m], v = a.v[m];
    const float mag = pm_speed_t<float>(u, v);
    e.Gx[m] = pm_force_t<float>(e, rho, gx, u, mag);
    e.Gy[m] = pm_force_t<float>(e, rho, gy, v, mag);
}

__global__ void k_pm_bary(const StepArgs a, const PmExtra e, const float *fl)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.nx) return;
    float f[9], rho, mx, my, u, v;
    pm_load_cell(fl + (long long)y * a.pitch + x, a.plane, f);
    pm_hydro_t<float>(f, rho, mx, my, u, v);        // (for the two momentum sums: rho is the stored one, as in the reference)
    const long long m = (long long)y * a.fpitch + x;
    rho = a.rho[m];
    e.ub[m] = pm_bary_t<float>(rho, mx, e.Gx[m]);
    e.vb[m] = pm_bary_t<float>(rho, my, e.Gy[m]);
}

__global__ void k_pm_feq(const StepArgs a, const PmExtra e, float *feq)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.nx) return;
    const long long m = (long long)y * a.fpitch + x;
    float q[9];
    pm_feq_t<float>(e, q, a.rho[m], e.ub[m], e.vb[m]);
    float *o = feq + (long long)y * a.pitch + x;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k * a.plane] = q[k];
}

__global__ void k_pm_collide(const StepArgs a, const PmExtra e, float *fl, const float *feq)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.nx) return;
    const long long o = (long long)y * a.pitch + x, m = (long long)y * a.fpitch + x;
    float f[9], q[9];
    pm_load_cell(fl + o, a.plane, f);
    pm_load_cell(feq + o, a.plane, q);
    pm_relax_t<float>(e, f, q, a.omega, a.rho[m], e.ub[m], e.vb[m], e.Gx[m], e.Gy[m]);
#pragma unroll
    for (int k = 0; k < 9; ++k) fl[o + k * a.plane] = f[k];
}

// move_open_bcs, in place behind lb_move: one thread per index i, grid = ceil(max(nx, ny) / 256): the cells (i, 0) and (i, ny-1) of the
// boundary rows, (0, i) and (nx-1, i) of the boundary columns between them.  Only interior cells are read and only boundary cells
// written: no race.
__device__ __forceinline__ void pm_bcs_cell(const StepArgs &a, float *f, int x, int y)
{
    const int xs = min(max(x, 1), a.nx - 2), ys = min(max(y, 1), a.ny - 2);
    float *to = f + (long long)y * a.pitch + x;
    const float *from = f + (long long)ys * a.pitch + xs;
#pragma unroll
    for (int k = 0; k < 9; ++k) to[k * a.plane] = from[k * a.plane];
}

__global__ void k_pm_move_bcs(const StepArgs a, float *f)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.nx) {
        pm_bcs_cell(a, f, i, 0);
        pm_bcs_cell(a, f, i, a.ny - 1);
    }
    if (i >= 1 && i <= a.ny - 2) {
        pm_bcs_cell(a, f, 0, i);
        pm_bcs_cell(a, f, a.nx - 1, i);
    }
}

}  // namespace
