// kernels_multifluid.h -- the kernels of multicomponent Shan-Chen fluids (LB_SEM_MULTIFLUID: the reference's
// LB_D2Q9/multicomponent_multiphase/multi.cl, driven as multi.py:729-803 does: per fluid move[_periodic] -> copy_streamed_onto_f ->
// move_open_bcs -> update_hydro_fluid, then Gx, Gy = 0 -> the additional forces -> update_bary_velocity -> per fluid update_feq_fluid
// -> collide_particles_fluid -> the additional collisions: about 6 NF + 4 + entries launches and as many host waits per step).
// Included by multifluid.cpp only (multifluid_launch.h: what the kernels, their host code and the handle share; host.h: what the other host units see).
//
// The step is NOT local to the cell after streaming: the interaction force on a cell reads the post-stream density of its eight
// neighbours.  Two forms of the step, bitwise equal (one body, mc_collide_lane).  The one-launch form:
//   k_mc_step<BC, NF, R, LAST>   the one-launch form of the lane-of-four plan (kernels_lane4.h): every wave gathers one row of every
//                                fluid and puts rho_i into LDS; the R owned rows run forces -> collide.  36 NF (R + 2) / R B read +
//                                36 NF B written per cell.
// The two-launch form:
//   k_mc_moments<BC, NF>         the gather, sums only, stores rho_i: 36 NF B read, 4 NF B written per cell
//   k_mc_collide<BC, NF, LAST>   gathers again, reads rho of the three rows around the cell (wrap or clamp on the INDEX, as the family
//                                says), forces -> u_b -> feq -> relaxation -> reactions in registers (multifluid_cell.h); LAST (a
//                                run's last step): u, v, Gx, Gy of every fluid and u_b, v_b as well
//   k_mc_hydro, k_mc_forces, k_mc_bary, k_mc_relax, k_mc_react    the reference's stages one by one, one cell per thread;
//                                multifluid_cell.h's functions, the same operations as the fused cell: bitwise equal to it.
//                                (move, move_open_bcs and update_feq_fluid are k_move, k_pm_move_bcs and k_pm_feq at epsilon = 1.)
// Halo cells outside the box: LB_BC_PERIODIC the wrapped cell; LB_BC_ZERO_GRADIENT the edge cell itself -- the reference clamps the
// stencil to [0, n-1] while the populations clamp to [1, n-2] (kernels_porous.h).
#pragma once
#include "kernels_porous.h"
#include "multifluid_cell.h"
#include "kernels_lane4.h"

namespace {

template <int BC, int NF>
__global__ __launch_bounds__(256) void k_mc_moments(const McArgs m)
{
    int x4, yl, ys, ym, yp;
    if (!lane_rows<BC>(m.a[0], x4, yl, ys, ym, yp)) return;
    const long long m0 = (long long)yl * m.a[0].fpitch;
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        f4a q[9];
        lane_gather<BC>(m.a[i], x4, ys, ym, yp, q);
        const f4a r4 = sum9(q);
        store4<false>(lane_ptr(m.a[i].rho + m0, x4), r4);
    }
}

// Stages 2-7 of a lane's four cells of row yl for every fluid, and the stores: q = the gathered populations, nb = rho around the
// cells (lane_nb_load's layout).  LAST: u, v, Gx, Gy of every fluid and u_b, v_b are stored as well; RHO: rho too (the one-launch
// step, whose rho never reached memory).  The one body of k_mc_collide and k_mc_step: they cannot differ in a bit.
template <int NF, bool LAST, bool RHO>
__device__ __forceinline__ void mc_collide_lane(const McArgs &m, int x4, int yl, f4a (&q)[NF][9], const float (&nb)[NF][3][6])
{
    const long long m0 = (long long)yl * m.a[0].fpitch;
    f4a g4x[NF], g4y[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        const PmExtra &e = m.e[i];
        g4x[i] = f4a{e.gx, e.gx, e.gx, e.gx};
        g4y[i] = f4a{e.gy, e.gy, e.gy, e.gy};
        if (e.fgx) {
            g4x[i] = g4x[i] + load4<false>(lane_ptr(e.fgx + m0, x4));
            g4y[i] = g4y[i] + load4<false>(lane_ptr(e.fgy + m0, x4));
        }
    }
    f4a r4[NF], u4[NF], v4[NF], Gx4[NF], Gy4[NF], ub4, vb4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f2a f[NF][9], rho[NF], mx[NF], my[NF], u[NF], v[NF], Gx[NF], Gy[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
#pragma unroll
            for (int k = 0; k < 9; ++k) f[i][k] = pair_of(q[i][k], h);
            mc_hydro_t<f2a>(f[i], rho[i], mx[i], my[i], u[i], v[i]);
            Gx[i] = pair_of(g4x[i], h) * rho[i];
            Gy[i] = pair_of(g4y[i], h) * rho[i];
        }
        for (int t = 0; t < m.n_inter; ++t) {
            const McInter it = m.inter[t];
            f2a p1[3][3], p2[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                float s1[4], s2[4];             // psi at the columns x - 1 ... x + 2 of the pair's first cell
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    float r1 = nb[0][r][2 * h + cc], r2 = r1;
#pragma unroll
                    for (int n = 1; n < NF; ++n) r1 = it.i == n ? nb[n][r][2 * h + cc] : r1;
#pragma unroll
                    for (int n = 0; n < NF; ++n) r2 = it.j == n ? nb[n][r][2 * h + cc] : r2;
                    s1[cc] = mc_psi(it.potential, it.par, r1);
                    s2[cc] = mc_psi(it.potential, it.par, r2);
                }
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) {
                    p1[r][cc] = f2a{s1[cc], s1[cc + 1]};
                    p2[r][cc] = f2a{s2[cc], s2[cc + 1]};
                }
            }
            mc_entry_force_t<f2a, NF>(it, p1, p2, Gx, Gy);
        }
        f2a sx = {0.f, 0.f}, sy = {0.f, 0.f}, rs = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NF; ++i) mc_bary_add_t<f2a>(f[i], rho[i], Gx[i], Gy[i], sx, sy, rs);
        const f2a ub = sx / rs, vb = sy / rs;
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            f2a eq[9];
            pm_feq_t<f2a>(m.e[i], eq, rho[i], ub, vb);
            mc_relax_t<f2a>(m.e[i], f[i], eq, m.a[i].omega, ub, vb, Gx[i], Gy[i]);
        }
        mc_react_t<f2a, NF>(m, f, rho);
#pragma unroll
        for (int i = 0; i < NF; ++i) {
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                if (h) q[i][k].zw = f[i][k];
                else q[i][k].xy = f[i][k];
            }
            if (h) { r4[i].zw = rho[i]; u4[i].zw = u[i]; v4[i].zw = v[i]; Gx4[i].zw = Gx[i]; Gy4[i].zw = Gy[i]; }
            else { r4[i].xy = rho[i]; u4[i].xy = u[i]; v4[i].xy = v[i]; Gx4[i].xy = Gx[i]; Gy4[i].xy = Gy[i]; }
        }
        if (h) { ub4.zw = ub; vb4.zw = vb; }
        else { ub4.xy = ub; vb4.xy = vb; }
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        store_planes(m.a[i], yl, x4, q[i]);
        if (LAST) {
            if (RHO) store4<false>(lane_ptr(m.a[i].rho + m0, x4), r4[i]);
            store4<false>(lane_ptr(m.a[i].u + m0, x4), u4[i]);
            store4<false>(lane_ptr(m.a[i].v + m0, x4), v4[i]);
            store4<false>(lane_ptr(m.e[i].Gx + m0, x4), Gx4[i]);
            store4<false>(lane_ptr(m.e[i].Gy + m0, x4), Gy4[i]);
            store4<false>(lane_ptr(m.e[i].ub + m0, x4), ub4);
            store4<false>(lane_ptr(m.e[i].vb + m0, x4), vb4);
        }
    }
}

template <int BC, int NF, bool LAST>
__global__ __launch_bounds__(256) void k_mc_collide(const McArgs m)
{
    int x4, yl, ys, ym, yp;
    if (!lane_rows<BC>(m.a[0], x4, yl, ys, ym, yp)) return;
    f4a q[NF][9];
    float nb[NF][3][6];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        lane_gather<BC>(m.a[i], x4, ys, ym, yp, q[i]);
        lane_nb_load<BC>(m.a[i].rho, m.a[0].fpitch, m.a[0].nx, m.a[0].ny, x4, yl, nb[i]);
    }
    mc_collide_lane<NF, LAST, false>(m, x4, yl, q, nb);
}

// ---- the one-launch step ------------------------------------------------------------------------------------------------------
// (kernels_lane4.h has the plan.)  One LDS row of rho_i per fluid and row of the tile.
template <int BC, int NF, int R, bool LAST>
__global__ __launch_bounds__(64 * (R + 2)) void k_mc_step(const McArgs m)
{
    __shared__ __attribute__((aligned(16))) float lds[NF][R + 2][LANE4_LDS_ROW];
    const StepArgs &a0 = m.a[0];
    const int lane = threadIdx.x, w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int x0 = blockIdx.x * 256, x4 = x0 + lane * 4;
    const int yo = blockIdx.y * R - 1 + w;              // the row this wave reads; owned: 1 <= w <= R and yo < ny
    int yl = yo;                                        // ... as a row of the box
    if (BC == LB_BC_PERIODIC) {
        if (yl < 0) yl = a0.ny - 1;
        if (yl >= a0.ny) yl -= a0.ny;
    }
    yl = min(max(yl, 0), a0.ny - 1);
    int ys = yl;
    if (BC == LB_BC_ZERO_GRADIENT) ys = min(max(yl, 1), a0.ny - 2);
    int ym = ys - 1, yp = ys + 1;
    if (BC == LB_BC_PERIODIC) {
        if (ym < 0) ym = a0.ny - 1;
        if (yp >= a0.ny) yp = 0;
    }
    const bool active = x4 < a0.fpitch;
    const int inside = min(256, a0.nx - x0);            // cells of the tile inside the box (<= 0: a tile of row padding)
    int xw = x0 - 1, xe = x0 + inside;
    if (xw < 0) xw = BC == LB_BC_PERIODIC ? a0.nx - 1 : 0;
    if (xe >= a0.nx) xe = BC == LB_BC_PERIODIC ? 0 : a0.nx - 1;
    f4a q[NF][9];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        if (active) {
            lane_gather<BC>(m.a[i], x4, ys, ym, yp, q[i]);
            *reinterpret_cast<f4a *>(&lds[i][w][4 + lane * 4]) = sum9(q[i]);
        }
    }
    if (inside > 0 && lane < 2) {
        // (behind the rows' own writes: the east halo takes the slot of the first padding cell, and a wave's LDS writes land in order)
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const float r = cell_rho<BC>(m.a[i], lane ? xe : xw, ys, ym, yp);
            lds[i][w][lane ? 4 + inside : 3] = r;
        }
    }
    __syncthreads();
    if (!active || w < 1 || w > R || yo >= a0.ny) return;
    float nb[NF][3][6];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float *row = &lds[i][w - 1 + r][4 + lane * 4];
            const f4a v = *reinterpret_cast<const f4a *>(row);
            nb[i][r][0] = row[-1];
            nb[i][r][1] = v.x; nb[i][r][2] = v.y; nb[i][r][3] = v.z; nb[i][r][4] = v.w;
            nb[i][r][5] = row[4];
        }
    mc_collide_lane<NF, LAST, true>(m, x4, yo, q, nb);
}

// ---- the reference's stages, one cell per thread: grid = (ceil(nx / 256), ny) ----------------------------------------------------
// (k_mc_forces and k_mc_bary write cell_xy out: the call moves their instruction text)
__global__ void k_mc_hydro(const StepArgs a)
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    float f[9], rho, mx, my, u, v;
    load_cell(a.src + (long long)y * a.pitch + x, a.plane, f);
    mc_hydro_t<float>(f, rho, mx, my, u, v);
    const long long o = (long long)y * a.fpitch + x;
    a.rho[o] = rho; a.u[o] = u; a.v[o] = v;
}

template <int BC>
__device__ __forceinline__ int mc_index(int i, int n)
{
    if (BC == LB_BC_PERIODIC) return i < 0 ? n - 1 : (i >= n ? 0 : i);
    return min(max(i, 0), n - 1);
}

template <int BC, int NF>
__global__ void k_mc_forces(const McArgs m)
{
    const StepArgs &a = m.a[0];
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.nx) return;
    const long long o = (long long)y * a.fpitch + x;
    long long at[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) at[r][c] = (long long)mc_index<BC>(y - 1 + r, a.ny) * a.fpitch + mc_index<BC>(x - 1 + c, a.nx);
    float Gx[NF], Gy[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        const PmExtra &e = m.e[i];
        float gx = e.gx, gy = e.gy;
        if (e.fgx) { gx = gx + e.fgx[o]; gy = gy + e.fgy[o]; }
        const float rho = m.a[i].rho[o];
        Gx[i] = gx * rho;
        Gy[i] = gy * rho;
    }
    for (int t = 0; t < m.n_inter; ++t) {
        const McInter it = m.inter[t];
        const float *r1 = m.a[0].rho, *r2 = m.a[0].rho;
#pragma unroll
        for (int n = 1; n < NF; ++n) {
            r1 = it.i == n ? m.a[n].rho : r1;
            r2 = it.j == n ? m.a[n].rho : r2;
        }
        float p1[3][3], p2[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                p1[r][c] = mc_psi(it.potential, it.par, r1[at[r][c]]);
                p2[r][c] = mc_psi(it.potential, it.par, r2[at[r][c]]);
            }
        mc_entry_force_t<float, NF>(it, p1, p2, Gx, Gy);
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        m.e[i].Gx[o] = Gx[i];
        m.e[i].Gy[o] = Gy[i];
    }
}

template <int NF>
__global__ void k_mc_bary(const McArgs m)
{
    const StepArgs &a = m.a[0];
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.nx) return;
    const long long o = (long long)y * a.fpitch + x;
    float sx = 0.f, sy = 0.f, rs = 0.f;
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        float f[9];
        load_cell(m.a[i].src + (long long)y * m.a[i].pitch + x, m.a[i].plane, f);
        mc_bary_add_t<float>(f, m.a[i].rho[o], m.e[i].Gx[o], m.e[i].Gy[o], sx, sy, rs);
    }
    const float ub = sx / rs, vb = sy / rs;
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        m.e[i].ub[o] = ub;
        m.e[i].vb[o] = vb;
    }
}

__global__ void k_mc_relax(const StepArgs a, const PmExtra e, float *fl, const float *feq)
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long o = (long long)y * a.pitch + x, c = (long long)y * a.fpitch + x;
    float f[9], q[9];
    load_cell(fl + o, a.plane, f);
    load_cell(feq + o, a.plane, q);
    mc_relax_t<float>(e, f, q, a.omega, e.ub[c], e.vb[c], e.Gx[c], e.Gy[c]);
#pragma unroll
    for (int k = 0; k < 9; ++k) fl[o + k * a.plane] = f[k];
}

template <int NF>
__global__ void k_mc_react(const McArgs m)
{
    const StepArgs &a = m.a[0];
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long c = (long long)y * a.fpitch + x;
    float f[NF][9], rho[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        load_cell(m.a[i].dst + (long long)y * m.a[i].pitch + x, m.a[i].plane, f[i]);
        rho[i] = m.a[i].rho[c];
    }
    mc_react_t<float, NF>(m, f, rho);
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        float *d = m.a[i].dst + (long long)y * m.a[i].pitch + x;
#pragma unroll
        for (int k = 0; k < 9; ++k) d[k * m.a[i].plane] = f[i][k];
    }
}

}  // namespace
