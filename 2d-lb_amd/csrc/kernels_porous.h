// kernels_porous.h -- the kernels of forced flow in a porous medium (LB_SEM_POROUS: the reference's
// LB_D2Q9/porous_media/single_component.cl, driven as single_component.py:679-751 does with one fluid: move[_periodic] ->
// copy_streamed_onto_f -> move_open_bcs -> update_hydro_pourous -> Gx, Gy = 0 -> the additional forces -> update_forces_pourous ->
// update_bary_velocity -> update_feq_pourous -> collide_particles_pourous, eleven launches and eleven host waits per step).  Included
// by porous.cpp only (porous_launch.h: what the kernels and their host code share; host.h: what the other host units see).
//   k_pm_step<BC, FIELD, LAST>   the fused step on the lane-of-four plan (kernels_lane4.h); FIELD: two 16-byte loads of the force field,
//                                the eight stages in registers (porous_cell.h); LAST (a run's last launch): seven more stores of rho, u,
//                                v, Gx, Gy, u_b, v_b.  72 B per cell and step, 80 B with a field, + 28 B on the last.
//   k_pm_move_bcs, k_pm_hydro, k_pm_forces, k_pm_bary, k_pm_feq, k_pm_collide   the reference's phases one by one; porous_cell.h's
//                                functions, the same operations as the fused cell: bitwise equal to it
// LB_BC_PERIODIC: the gather wraps.  LB_BC_ZERO_GRADIENT: cell (x, y) is, after move + move_open_bcs, a copy of the
// post-stream interior cell (xs, ys) = (clamp(x, 1, nx-2), clamp(y, 1, ny-2)), so in pull form it gathers link k from
// (xs - c_kx, ys - c_ky): the SOURCE cell is clamped.  In y the clamp is wave-uniform -- rows 0 and ny-1 simply gather what rows 1 and
// ny-2 gather, no second load; in x the cell x = 0 takes the gathered cell x = 1 of its own lane, the cell x = nx-1 the gathered cell
// nx-2: a select where that is in the lane, nine scalar loads on that one lane where nx-1 is a lane's first cell.  The gather itself is
// the one without a wrap (it reads row padding beside the box: inside the allocation, replaced by the selects): lane_rows, clamp_x.
#pragma once
#include "porous_cell.h"
#include "kernels_lane4.h"

namespace {

// stages 3-8 of a lane's four gathered cells as two pairs (porous_cell.h, T = f2a), in place; g4x, g4y: the body force of the cells
__device__ __forceinline__ void pm_collide_row(const PmExtra &e, float omega, f4a (&q)[9], f4a g4x, f4a g4y, f4a &r4, f4a &u4,
                                               f4a &v4, f4a &Gx4, f4a &Gy4, f4a &ub4, f4a &vb4)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f2a f[9], eq[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = pair_of(q[k], h);
        f2a rho, mx, my, u, v;
        pm_hydro_t<f2a>(f, rho, mx, my, u, v);
        const f2a mag = pm_speed_t<f2a>(u, v);
        const f2a Gx = pm_force_t<f2a>(e, rho, pair_of(g4x, h), u, mag);
        const f2a Gy = pm_force_t<f2a>(e, rho, pair_of(g4y, h), v, mag);
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

template <int BC, bool FIELD, bool LAST>
__global__ __launch_bounds__(256) void k_pm_step(const StepArgs a, const PmExtra e)
{
    // (lane_rows and the nine stores written out: through the calls the ZERO_GRADIENT form computes yp in front of ym, the plane offsets
    //  are shared with the gather's, and the instruction text moves)
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int yl = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);
    if (x4 >= a.fpitch || yl >= a.ny) return;
    int ys = yl;
    if (BC == LB_BC_ZERO_GRADIENT) ys = min(max(yl, 1), a.ny - 2);
    int ym = ys - 1, yp = ys + 1;
    if (BC == LB_BC_PERIODIC) {
        if (ym < 0) ym = a.ny - 1;
        if (yp >= a.ny) yp = 0;
    }
    f4a q[9];
    lane_gather<BC, false>(a, x4, ys, ym, yp, q);
    const long long m0 = (long long)yl * a.fpitch;
    f4a g4x = {e.gx, e.gx, e.gx, e.gx}, g4y = {e.gy, e.gy, e.gy, e.gy};
    if (FIELD) {
        g4x = g4x + load4<false>(lane_ptr(e.fgx + m0, x4));
        g4y = g4y + load4<false>(lane_ptr(e.fgy + m0, x4));
    }
    if (BC == LB_BC_ZERO_GRADIENT) clamp_x(a, x4, ys, q);      // (behind the force loads: they are in flight with the gather)
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
__global__ void k_pm_hydro(const StepArgs a)
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    float f[9], rho, mx, my, u, v;
    load_cell(a.src + (long long)y * a.pitch + x, a.plane, f);
    pm_hydro_t<float>(f, rho, mx, my, u, v);
    const long long m = (long long)y * a.fpitch + x;
    a.rho[m] = rho; a.u[m] = u; a.v[m] = v;
}

__global__ void k_pm_forces(const StepArgs a, const PmExtra e)
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
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
    int x, y;
    if (!cell_xy(a, x, y)) return;
    float f[9], rho, mx, my, u, v;
    load_cell(fl + (long long)y * a.pitch + x, a.plane, f);
    pm_hydro_t<float>(f, rho, mx, my, u, v);        // (for the two momentum sums: rho is the stored one, as in the reference)
    const long long m = (long long)y * a.fpitch + x;
    rho = a.rho[m];
    e.ub[m] = pm_bary_t<float>(rho, mx, e.Gx[m]);
    e.vb[m] = pm_bary_t<float>(rho, my, e.Gy[m]);
}

__global__ void k_pm_feq(const StepArgs a, const PmExtra e, float *feq)
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long m = (long long)y * a.fpitch + x;
    float q[9];
    pm_feq_t<float>(e, q, a.rho[m], e.ub[m], e.vb[m]);
    float *o = feq + (long long)y * a.pitch + x;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k * a.plane] = q[k];
}

__global__ void k_pm_collide(const StepArgs a, const PmExtra e, float *fl, const float *feq)
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long o = (long long)y * a.pitch + x, m = (long long)y * a.fpitch + x;
    float f[9], q[9];
    load_cell(fl + o, a.plane, f);
    load_cell(feq + o, a.plane, q);
    pm_relax_t<float>(e, f, q, a.omega, a.rho[m], e.ub[m], e.vb[m], e.Gx[m], e.Gy[m]);
#pragma unroll
    for (int k = 0; k < 9; ++k) fl[o + k * a.plane] = f[k];
}

// move_open_bcs, in place behind lb_move (edge_walk, kernels_lane4.h): an edge cell becomes a copy of its interior neighbour.  Only
// interior cells are read and only boundary cells written: no race.
struct PmEdge {
    __device__ __forceinline__ void edge_cell(const StepArgs &a, float *f, int x, int y) const
    {
        const int xs = min(max(x, 1), a.nx - 2), ys = min(max(y, 1), a.ny - 2);
        float *to = f + (long long)y * a.pitch + x;
        const float *from = f + (long long)ys * a.pitch + xs;
#pragma unroll
        for (int k = 0; k < 9; ++k) to[k * a.plane] = from[k * a.plane];
    }
};

__global__ void k_pm_move_bcs(const StepArgs a, float *f) { edge_walk(a, f, PmEdge{}); }

}  // namespace
