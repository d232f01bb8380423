// kernels_rocket.h -- the kernels of surfactant-propelled colonies (LB_SEM_ROCKET: the reference's LB_D2Q9/rocket_yeast/
// rocket_yeast.cl and rocket_yeast_forces_only.cl, driven as rocket_yeast.py:469-483 does: move_periodic -> copy -> update_hydro ->
// update_u_and_v -> update_psi -> update_pseudo_force -> update_feq -> collide_particles, nine launches, nine host waits and a full
// copy of f per step).  Included by rocket.cpp only (rocket_launch.h: what the kernels and their host code share; host.h: what the other host units see).
//
// Two scalar lattices in a periodic box, the population p and the surfactant c.  The velocity that advects both is a D2Q9 stencil over
// the surfactant (MODE = LB_ROCKET_FLOW) or the sum of two stencil forces (LB_ROCKET_FORCES), so the step is NOT local to the cell
// after streaming: it reads two OPERANDS at the eight neighbours -- A from rho_c (FLOW: rho_c itself; FORCES: S(rho_c)) and B from
// rho_p (FLOW: psi(rho_p); FORCES: rho_p itself).  Three forms, bitwise equal (one body, ry_collide_lane, and rocket_cell.h):
// All three are on the lane-of-four plan, and the first on its one-launch form, of kernels_lane4.h:
//   k_ry_step<MODE, R, LAST>     one launch per step: every wave gathers one row of both lattices and puts A and B of its 256 cells into
//                                LDS; the R owned rows run stages 3-5 and store.  72 (R + 2) / R B read + 72 B written per cell.
//   k_ry_moments                 the two-launch form: the gather, sums only, stores rho_p and rho_c: 72 B read, 8 B written per cell
//   k_ry_collide<MODE, LAST>     gathers again, reads both densities of the three rows around the cell (wrap on the INDEX), forms the
//                                operands and runs stages 3-5; LAST (a run's last step): u, v, psi / S and the forces as well
//   k_ry_velocity, k_ry_forces, k_ry_relax    the reference's stages 3 and 5 one by one, one cell per thread (move, update_hydro and
//                                update_feq are the scalar lattice's k_move, k_ad_hydro and k_ad_feq: the same operations)
#pragma once
#include "rocket_cell.h"
#include "kernels_lane4.h"

namespace {

__global__ __launch_bounds__(256) void k_ry_moments(const RyArgs m)
{
    int x4, yl, ys, ym, yp;
    if (!lane_rows<LB_BC_PERIODIC>(m.a[0], x4, yl, ys, ym, yp)) return;
    const long long m0 = (long long)yl * m.a[0].fpitch;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        f4a q[9];
        lane_gather<LB_BC_PERIODIC>(m.a[i], x4, ys, ym, yp, q);
        store4<false>(lane_ptr(m.a[i].rho + m0, x4), sum9(q));
    }
}

// Stages 2-5 of a lane's four cells of row yl for both lattices, and the stores: q = the gathered populations, na / nb = the operands A
// and B around the cells (lane_nb_load's layout).  LAST: u, v (to both members), psi / S and the forces are stored as well; RHO: both
// densities too (the one-launch step, whose densities never reached memory).  The one body of k_ry_collide and k_ry_step.
template <int MODE, bool LAST, bool RHO>
__device__ __forceinline__ void ry_collide_lane(const RyArgs &m, int x4, int yl, f4a (&q)[2][9], const float (&na)[3][6], const float (&nb)[3][6])
{
    const long long m0 = (long long)yl * m.a[0].fpitch;
    f4a rp4, rc4, u4, v4, Fx4, Fy4, Sx4, Sy4, op4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f2a fp[9], fc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            fp[k] = pair_of(q[0][k], h);
            fc[k] = pair_of(q[1][k], h);
        }
        const f2a rho_p = ad_rho_t<f2a>(fp[0], fp[1], fp[2], fp[3], fp[4], fp[5], fp[6], fp[7], fp[8]);
        const f2a rho_c = ad_rho_t<f2a>(fc[0], fc[1], fc[2], fc[3], fc[4], fc[5], fc[6], fc[7], fc[8]);
        f2a pa[3][3], pb[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                pa[r][cc] = f2a{na[r][2 * h + cc], na[r][2 * h + cc + 1]};
                pb[r][cc] = f2a{nb[r][2 * h + cc], nb[r][2 * h + cc + 1]};
            }
        f2a u, v, Fx, Fy, Sx = {0.f, 0.f}, Sy = {0.f, 0.f};
        if (MODE == LB_ROCKET_FLOW) {
            ry_marangoni_t<f2a>(m, pa, u, v);
            ry_pseudo_force_t<f2a>(m, pb, Fx, Fy);
        } else {
            ry_marangoni_t<f2a>(m, pa, Sx, Sy);
            ry_pressure_force_t<f2a>(m, pb, Fx, Fy);
            u = Fx + Sx;
            v = Fy + Sy;
        }
        f2a ep[9], ec[9];
        ry_feq_t<f2a>(ep, rho_p, u, v);
        ry_feq_t<f2a>(ec, rho_c, u, v);
        ry_relax_pop_t<f2a, MODE>(m, fp, ep, m.a[0].omega, rho_p, Fx, Fy);
        ry_relax_surf_t<f2a>(m, fc, ec, m.a[1].omega, rho_p);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (h) { q[0][k].zw = fp[k]; q[1][k].zw = fc[k]; }
            else { q[0][k].xy = fp[k]; q[1][k].xy = fc[k]; }
        }
        const f2a op = MODE == LB_ROCKET_FLOW ? pb[1][1] : pa[1][1];
        if (h) { rp4.zw = rho_p; rc4.zw = rho_c; u4.zw = u; v4.zw = v; Fx4.zw = Fx; Fy4.zw = Fy; Sx4.zw = Sx; Sy4.zw = Sy; op4.zw = op; }
        else { rp4.xy = rho_p; rc4.xy = rho_c; u4.xy = u; v4.xy = v; Fx4.xy = Fx; Fy4.xy = Fy; Sx4.xy = Sx; Sy4.xy = Sy; op4.xy = op; }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        store_planes(m.a[i], yl, x4, q[i]);
        if (LAST) {
            if (RHO) store4<false>(lane_ptr(m.a[i].rho + m0, x4), i ? rc4 : rp4);
            store4<false>(lane_ptr(m.a[i].u + m0, x4), u4);
            store4<false>(lane_ptr(m.a[i].v + m0, x4), v4);
        }
    }
    if (LAST) {
        store4<false>(lane_ptr(m.op + m0, x4), op4);
        store4<false>(lane_ptr(m.Fx + m0, x4), Fx4);
        store4<false>(lane_ptr(m.Fy + m0, x4), Fy4);
        if (MODE == LB_ROCKET_FORCES) {
            store4<false>(lane_ptr(m.Sx + m0, x4), Sx4);
            store4<false>(lane_ptr(m.Sy + m0, x4), Sy4);
        }
    }
}

template <int MODE, bool LAST>
__global__ __launch_bounds__(256) void k_ry_collide(const RyArgs m)
{
    int x4, yl, ys, ym, yp;
    if (!lane_rows<LB_BC_PERIODIC>(m.a[0], x4, yl, ys, ym, yp)) return;
    f4a q[2][9];
    float na[3][6], nb[3][6];
    lane_gather<LB_BC_PERIODIC>(m.a[0], x4, ys, ym, yp, q[0]);
    lane_gather<LB_BC_PERIODIC>(m.a[1], x4, ys, ym, yp, q[1]);
    lane_nb_load<LB_BC_PERIODIC>(m.a[1].rho, m.a[0].fpitch, m.a[0].nx, m.a[0].ny, x4, yl, na);
    lane_nb_load<LB_BC_PERIODIC>(m.a[0].rho, m.a[0].fpitch, m.a[0].nx, m.a[0].ny, x4, yl, nb);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            na[r][c] = ry_op_a<MODE>(m, na[r][c]);
            nb[r][c] = ry_op_b<MODE>(m, nb[r][c]);
        }
    ry_collide_lane<MODE, LAST, false>(m, x4, yl, q, na, nb);
}

// ---- the one-launch step (kernels_lane4.h has the plan and the LDS row) -----------------------------------------------------------
// What a wave puts into LDS is not a density but the operands A and B of its cells: two LDS rows per row of the tile.
template <int MODE, int R, bool LAST>
__global__ __launch_bounds__(64 * (R + 2)) void k_ry_step(const RyArgs m)
{
    __shared__ __attribute__((aligned(16))) float lds[2][R + 2][LANE4_LDS_ROW];
    const StepArgs &a0 = m.a[0];
    const int lane = threadIdx.x, w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int x0 = blockIdx.x * 256, x4 = x0 + lane * 4;
    const int yo = blockIdx.y * R - 1 + w;              // the row this wave reads; owned: 1 <= w <= R and yo < ny
    int yl = yo;                                        // ... as a row of the box
    if (yl < 0) yl = a0.ny - 1;
    if (yl >= a0.ny) yl -= a0.ny;
    yl = min(max(yl, 0), a0.ny - 1);                    // (rows past the halo of the last workgroup: in the box, never used)
    int ym = yl - 1, yp = yl + 1;
    if (ym < 0) ym = a0.ny - 1;
    if (yp >= a0.ny) yp = 0;
    const bool active = x4 < a0.fpitch;
    const int inside = min(256, a0.nx - x0);            // cells of the tile inside the box (<= 0: a tile of row padding)
    int xw = x0 - 1, xe = x0 + inside;
    if (xw < 0) xw = a0.nx - 1;
    if (xe >= a0.nx) xe = 0;
    f4a q[2][9];
    if (active) {
        lane_gather<LB_BC_PERIODIC>(m.a[0], x4, yl, ym, yp, q[0]);
        lane_gather<LB_BC_PERIODIC>(m.a[1], x4, yl, ym, yp, q[1]);
        const f4a rp = sum9(q[0]), rc = sum9(q[1]);
        f4a A, B;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            A[j] = ry_op_a<MODE>(m, rc[j]);
            B[j] = ry_op_b<MODE>(m, rp[j]);
        }
        *reinterpret_cast<f4a *>(&lds[0][w][4 + lane * 4]) = A;
        *reinterpret_cast<f4a *>(&lds[1][w][4 + lane * 4]) = B;
    }
    if (inside > 0 && lane < 2) {
        // (behind the rows' own writes: the east halo takes the slot of the first padding cell, and a wave's LDS writes land in order)
        const int xh = lane ? xe : xw;
        const float rc = cell_rho<LB_BC_PERIODIC>(m.a[1], xh, yl, ym, yp), rp = cell_rho<LB_BC_PERIODIC>(m.a[0], xh, yl, ym, yp);
        lds[0][w][lane ? 4 + inside : 3] = ry_op_a<MODE>(m, rc);
        lds[1][w][lane ? 4 + inside : 3] = ry_op_b<MODE>(m, rp);
    }
    __syncthreads();
    if (!active || w < 1 || w > R || yo >= a0.ny) return;
    float na[3][6], nb[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float *ra = &lds[0][w - 1 + r][4 + lane * 4], *rb = &lds[1][w - 1 + r][4 + lane * 4];
        const f4a va = *reinterpret_cast<const f4a *>(ra), vb = *reinterpret_cast<const f4a *>(rb);
        na[r][0] = ra[-1]; na[r][1] = va.x; na[r][2] = va.y; na[r][3] = va.z; na[r][4] = va.w; na[r][5] = ra[4];
        nb[r][0] = rb[-1]; nb[r][1] = vb.x; nb[r][2] = vb.y; nb[r][3] = vb.z; nb[r][4] = vb.w; nb[r][5] = rb[4];
    }
    ry_collide_lane<MODE, LAST, true>(m, x4, yo, q, na, nb);
}

// ---- the reference's stages, one cell per thread: grid = (ceil(nx / 256), ny) ----------------------------------------------------
// the operand OP (0 = A from rho_c, 1 = B from rho_p) at the eight neighbours and the cell itself, from the stored densities
template <int MODE, int OP>
__device__ __forceinline__ void ry_operand_3x3(const RyArgs &m, int x, int y, float (&p)[3][3])
{
    const StepArgs &a = m.a[0];
    const float *rho = OP ? m.a[0].rho : m.a[1].rho;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int yy = y - 1 + r, xx = x - 1 + c;
            yy = yy < 0 ? a.ny - 1 : (yy >= a.ny ? 0 : yy);
            xx = xx < 0 ? a.nx - 1 : (xx >= a.nx ? 0 : xx);
            const float d = rho[(long long)yy * a.fpitch + xx];
            p[r][c] = OP ? ry_op_b<MODE>(m, d) : ry_op_a<MODE>(m, d);
        }
}

// update_u_and_v.  FLOW: the stencil over rho_c; FORCES: the sum of the two stored forces.  Both members receive it.
template <int MODE>
__global__ void k_ry_velocity(const RyArgs m)
{
    const StepArgs &a = m.a[0];
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long o = (long long)y * a.fpitch + x;
    float u, v;
    if (MODE == LB_ROCKET_FLOW) {
        float p[3][3];
        ry_operand_3x3<MODE, 0>(m, x, y, p);
        ry_marangoni_t<float>(m, p, u, v);
    } else {
        u = m.Fx[o] + m.Sx[o];
        v = m.Fy[o] + m.Sy[o];
    }
    m.a[0].u[o] = u; m.a[0].v[o] = v;
    m.a[1].u[o] = u; m.a[1].v[o] = v;
}

// FLOW: update_psi + update_pseudo_force.  FORCES: update_surf_tension + update_surface_forces + update_pressure_force.
template <int MODE>
__global__ void k_ry_forces(const RyArgs m)
{
    const StepArgs &a = m.a[0];
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long o = (long long)y * a.fpitch + x;
    float pb[3][3], Fx, Fy;
    ry_operand_3x3<MODE, 1>(m, x, y, pb);
    if (MODE == LB_ROCKET_FLOW) {
        ry_pseudo_force_t<float>(m, pb, Fx, Fy);
        m.op[o] = pb[1][1];
    } else {
        float pa[3][3], Sx, Sy;
        ry_operand_3x3<MODE, 0>(m, x, y, pa);
        ry_marangoni_t<float>(m, pa, Sx, Sy);
        ry_pressure_force_t<float>(m, pb, Fx, Fy);
        m.op[o] = pa[1][1];
        m.Sx[o] = Sx; m.Sy[o] = Sy;
    }
    m.Fx[o] = Fx; m.Fy[o] = Fy;
}

// collide_particles: both lattices at a[i].dst (the launcher puts the current lattice there) relaxed in place towards the stored feq,
// from the stored rho_p and F
template <int MODE>
__global__ void k_ry_relax(const RyArgs m, const float *feq_p, const float *feq_c)
{
    const StepArgs &a = m.a[0];
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long o = (long long)y * a.pitch + x, c = (long long)y * a.fpitch + x, S = a.plane;
    float *fp = m.a[0].dst + o, *fc = m.a[1].dst + o;
    float f[9], e[9];
    const float rho_p = m.a[0].rho[c];
#pragma unroll
    for (int k = 0; k < 9; ++k) { f[k] = fp[k * S]; e[k] = feq_p[o + k * S]; }
    float Fx = 0.f, Fy = 0.f;
    if (MODE == LB_ROCKET_FLOW) { Fx = m.Fx[c]; Fy = m.Fy[c]; }
    ry_relax_pop_t<float, MODE>(m, f, e, m.a[0].omega, rho_p, Fx, Fy);
#pragma unroll
    for (int k = 0; k < 9; ++k) fp[k * S] = f[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) { f[k] = fc[k * S]; e[k] = feq_c[o + k * S]; }
    ry_relax_surf_t<float>(m, f, e, m.a[1].omega, rho_p);
#pragma unroll
    for (int k = 0; k < 9; ++k) fc[k * S] = f[k];
}

}  // namespace
