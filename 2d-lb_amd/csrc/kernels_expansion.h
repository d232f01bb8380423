// kernels_expansion.h -- the kernels of noisy strains on a shared nutrient (the reference's LB_D2Q9/D2Q9_multifield_diffusion.cl, driven
// as advecting_range_expansion/stochastic_nutrients.py:478-496 does: move + copy_buffer -> move_bcs (`pass`) -> update_hydro ->
// update_feq -> collide_particles, six launches and six host waits per step, and a refill of the random_normal buffer).  Included by
// expansion.cpp only (expansion_launch.h: what the kernels and their host code share; host.h: what the other host units see).
//
// NP = 1 ... 3 strains and the nutrient behind them, NP + 1 scalar lattices (LB_SEM_DIFFUSION) in one box, LB_BC_OPEN (the reference's
// box: a link that would enter from outside keeps the member's edge state, kernels_scalar.h) or LB_BC_PERIODIC.
//   k_ex_step<BC, NP, RHO>   the fused step on the lane-of-four plan (kernels_lane4.h): gathers every member, rho_i = sum f cut at
//                            zero_cutoff, one load each of u and v for all, per noisy strain ONE Philox call for the lane (four normals
//                            in registers, scalar_cell.h: ad_lane_normals; a strain with Dg == 0 draws nothing: a wave-uniform branch),
//                            react_i = (G_i rho_i) c + sqrt((Dg_i rho_i) c) z + ((Dg_i c) / 4)(z z - 1), the strains in order, the
//                            nutrient - sum react_i behind them, the floor, the stores; RHO: every member's cut rho as well.
//                            72 (NP + 1) B + 8 B per cell and step.
//   k_ex_hydro<NF>, k_ex_collide<NP>   the reference's stages one cell per thread (move and update_feq are the scalar lattice's k_move
//                            and k_ad_feq).  They keep the un-fused order -- feq stored, then f (1 - omega) + omega feq -- and so round
//                            differently from the fused cell, where omega enters through rho: held to it by the contract's tolerance.
#pragma once
#include "scalar_cell.h"
#include "expansion_launch.h"
#include "kernels_lane4.h"      // lane_gather, ad_edge_gather, store_planes, cell_xy

namespace {

// moments, cutoffs, the strains in order, the nutrient: a lane's four gathered cells of every member as two pairs, in place
template <int NP>
__device__ __forceinline__ void ex_collide_row(f4a (&q)[NP + 1][9], f4a u4, f4a v4, const ExArgs &m, const float (&z)[NP][4],
                                               f4a (&r4)[NP + 1])
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f2a ux = pair_of(u4, h), uy = pair_of(v4, h);
        f2a rho[NP + 1];
#pragma unroll
        for (int i = 0; i <= NP; ++i) {
            const f2a sum = ad_rho_t<f2a>(pair_of(q[i][0], h), pair_of(q[i][1], h), pair_of(q[i][2], h), pair_of(q[i][3], h),
                                          pair_of(q[i][4], h), pair_of(q[i][5], h), pair_of(q[i][6], h), pair_of(q[i][7], h),
                                          pair_of(q[i][8], h));
            rho[i] = ex_cut(sum, m.cut);
            if (h) r4[i].zw = rho[i];
            else r4[i].xy = rho[i];
        }
        const f2a c = rho[NP];
        f2a eaten = lb_splat<f2a>(0.f);
#pragma unroll
        for (int i = 0; i <= NP; ++i) {
            f2a react;
            if (i == NP) react = eaten;
            else {
                if (m.Dg[i] != 0.f) react = ex_react_t<f2a, true>(m.G[i], m.Dg[i], rho[i], c, f2a{z[i][2 * h], z[i][2 * h + 1]});
                else react = ex_react_t<f2a, false>(m.G[i], 0.f, rho[i], c, lb_splat<f2a>(0.f));
                eaten = eaten - react;
            }
            f2a f[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) f[k] = pair_of(q[i][k], h);
            ex_relax_t<f2a>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], m.a[i].omega, m.cut, rho[i], ux, uy, react);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                if (h) q[i][k].zw = f[k];
                else q[i][k].xy = f[k];
            }
        }
    }
}

template <int BC, int NP, bool RHO>
__global__ __launch_bounds__(256) void k_ex_step(const ExArgs m)
{
    const StepArgs &g = m.a[0];                 // the set's geometry, and the imposed velocity every member reads
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int yl = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);
    if (x4 >= g.fpitch || yl >= g.ny) return;
    int ym = yl - 1, yp = yl + 1;               // source rows of the cy = +1 / cy = -1 links
    if (BC == LB_BC_PERIODIC) {
        if (ym < 0) ym = g.ny - 1;
        if (yp >= g.ny) yp = 0;
    }
    f4a q[NP + 1][9], r4[NP + 1];
#pragma unroll
    for (int i = 0; i <= NP; ++i) {
        lane_gather<BC>(m.a[i], x4, yl, ym, yp, q[i]);
        if (BC == LB_BC_OPEN) ad_edge_gather(m.edge[i], g.fpitch, g.nx, g.ny, x4, yl, q[i]);
    }
    const long long m0 = (long long)yl * g.fpitch;
    const f4a u4 = load4<false>(lane_ptr((const float *)g.u + m0, x4));
    const f4a v4 = load4<false>(lane_ptr((const float *)g.v + m0, x4));
    float z[NP][4];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (m.Dg[i] != 0.f) ad_lane_normals(m.seed[i], x4, yl, m.t[i], z[i]);
        else z[i][0] = z[i][1] = z[i][2] = z[i][3] = 0.f;
    }
    ex_collide_row<NP>(q, u4, v4, m, z, r4);
#pragma unroll
    for (int i = 0; i <= NP; ++i) {
        store_planes(m.a[i], yl, x4, q[i]);
        if (RHO) store4<false>(lane_ptr(m.a[i].rho + m0, x4), r4[i]);
    }
}

// ---- the reference's stages, one cell per thread: grid = (ceil(nx / 256), ny) ----------------------------------------------------
// update_hydro: every member's rho = sum f of the lattice at a[i].src, cut
template <int NF>
__global__ void k_ex_hydro(const ExArgs m)
{
    const StepArgs &g = m.a[0];
    int x, y;
    if (!cell_xy(g, x, y)) return;
    const long long o = (long long)y * g.pitch + x, c = (long long)y * g.fpitch + x, S = g.plane;
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        const float *f = m.a[i].src + o;
        const float sum = ad_rho_t<float>(f[0], f[S], f[2 * S], f[3 * S], f[4 * S], f[5 * S], f[6 * S], f[7 * S], f[8 * S]);
        m.a[i].rho[c] = ex_cut(sum, m.cut);
    }
}

// collide_particles: every member at a[i].dst (the launcher puts the current lattice there) relaxed in place towards the stored feq,
// from the stored densities; z from the strain's supplied field where there is one, else from its stream
template <int NP>
__global__ void k_ex_collide(const ExArgs m)
{
    const StepArgs &g = m.a[0];
    int x, y;
    if (!cell_xy(g, x, y)) return;
    const long long o = (long long)y * g.pitch + x, c = (long long)y * g.fpitch + x, S = g.plane;
    const float cn = m.a[NP].rho[c];
    float eaten = 0.f;
#pragma unroll
    for (int i = 0; i <= NP; ++i) {
        const float rho = i == NP ? cn : m.a[i].rho[c];
        float react;
        if (i == NP) react = eaten;
        else {
            if (m.Dg[i] != 0.f) {
                const float z = m.field[i] ? m.field[i][(long long)y * g.nx + x] : ad_cell_normal(m.seed[i], x, y, m.t[i]);
                react = ex_react_t<float, true>(m.G[i], m.Dg[i], rho, cn, z);
            } else {
                react = ex_react_t<float, false>(m.G[i], 0.f, rho, cn, 0.f);
            }
            eaten = eaten - react;
        }
        float *f = m.a[i].dst + o;
        const float *feq = m.feq[i] + o;
        const float omega = m.a[i].omega, keep = 1.f - omega;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float relax = lb_fma(f[k * S], keep, omega * feq[k * S]);
            f[k * S] = ex_floor(lb_fma(lb_w9(k), react, relax), rho, m.cut);
        }
    }
}

}  // namespace
