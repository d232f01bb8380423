// kernels_multifield.h -- the kernels of coupled scalar lattices (LB_SEM_MULTIFIELD: the reference's LB_D2Q9/D2Q9_multifield_fisher.cl,
// driven as advecting_range_expansion/deterministic_fisher_waves.py:436-450 does: move + copy_buffer -> move_bcs -> update_hydro ->
// update_feq -> collide_particles, five launches and five host waits per step, each looping over the fields in every work-item).
// Included by multifield.cpp only (multifield_launch.h: what the kernels and their host code share; host.h: what the other host units see).
//   k_mf_step<BC, NF, RHO>   the fused step of NF fields on the lane-of-four plan (kernels_lane4.h): u and v loaded once for all fields,
//                            rho of every field when asked: 72 NF + 8 B per cell and step.  Every field's gathered populations are
//                            live before any collision -- rho_tot comes first --: 36 registers per field.  The cell arithmetic is
//                            scalar_cell.h's: with one field the bits of k_ad_step.
//   k_mf_move_bcs            the un-fused move_bcs of LB_BC_BOX, in place, edge cells only
//   k_mf_collide<NF>         the un-fused collide_particles: stored feq and rho, rho_tot summed over the fields' stored rho in order
// (lb_move, lb_update_hydro, lb_update_feq, lb_init_pop reuse k_move / k_ad_hydro / k_ad_feq: per field they are the same kernels.)
// LB_BC_BOX, the reference's closed box: the gather is the one without a wrap (it reads row padding and ghost rows beside the box:
// inside the allocation, never used) and every link that entered from outside is replaced by move_bcs's rule, which reads
// post-stream links of the same cell -- the lane has them in registers.  Two links per corner are neither streamed nor bounced:
// they come from the field's corner state.
#pragma once
#include "scalar_cell.h"
#include "multifield_launch.h"
#include "kernels_lane4.h"

namespace {

// move_bcs of D2Q9_multifield_fisher.cl for one cell (w, e, s, n: it lies in column 0 / nx-1, row 0 / ny-1); st: the eight corner
// links in the ABI's order -- f6, f8 of (0,0), f5, f7 of (nx-1,0), f5, f7 of (0,ny-1), f6, f8 of (nx-1,ny-1).  Every right-hand
// side is a post-stream value of the cell, read before anything is written, as the kernel reads f1 ... f8 first.
struct MfBox {
    __device__ __forceinline__ void rule(Cell &c, bool w, bool e, bool s, bool n, const float *st) const
    {
        const float f1 = c.f1, f2 = c.f2, f3 = c.f3, f4 = c.f4, f5 = c.f5, f6 = c.f6, f7 = c.f7, f8 = c.f8;
        if (w) c.f1 = f3;
        if (e) c.f3 = f1;
        if (s) c.f2 = f4;
        if (n) c.f4 = f2;
        // a diagonal link enters from outside through either wall its velocity points away from; bounced except in the corner whose
        // other wall it runs along
        if (w || s) c.f5 = (w && n) ? st[4] : ((s && e) ? st[2] : f7);
        if (e || n) c.f7 = (e && s) ? st[3] : ((n && w) ? st[5] : f5);
        if (e || s) c.f6 = (s && w) ? st[0] : ((e && n) ? st[6] : f8);
        if (w || n) c.f8 = (w && s) ? st[1] : ((n && e) ? st[7] : f6);
    }
};

// moments of every field, rho_tot, then equilibrium, relaxation and growth of every field: a lane's four cells as two pairs, in
// place.  A field with G = 0 skips the growth term (wave-uniform): plain relaxation.
template <int NF>
__device__ __forceinline__ void mf_collide_row(f4a (&q)[NF][9], f4a u4, f4a v4, const MfArgs &m, f4a (&r4)[NF])
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f2a ux = pair_of(u4, h), uy = pair_of(v4, h);
        f2a rho[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            f2a f[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) f[k] = pair_of(q[i][k], h);
            rho[i] = ad_rho_t<f2a>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]);
        }
        f2a rho_tot = rho[0];
#pragma unroll
        for (int i = 1; i < NF; ++i) rho_tot = rho_tot + rho[i];
        const f2a room = lb_splat<f2a>(1.f) - rho_tot;
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            f2a f[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) f[k] = pair_of(q[i][k], h);
            ad_relax_t<f2a, false>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], m.a[i].omega, 0.f, rho[i], ux, uy);
            if (m.G[i] != 0.f) ad_grow_t<f2a>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], m.G[i], rho[i], room);
            if (h) r4[i].zw = rho[i];
            else r4[i].xy = rho[i];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                if (h) q[i][k].zw = f[k];
                else q[i][k].xy = f[k];
            }
        }
    }
}

// (lane_rows, lane_gather and the nine stores written out: through the calls the BOX form tests its two bounds at once, the diagnostic
// build orders the gather differently, the plane offsets are shared with the gather's, and the instruction text moves)
template <int BC, int NF, bool RHO>
__global__ __launch_bounds__(256) void k_mf_step(const MfArgs m)
{
    const StepArgs &g = m.a[0];                 // the set's geometry, and the imposed velocity every field reads
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int yl = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);
    if (x4 >= g.fpitch || yl >= g.ny) return;
    int ym = yl - 1, yp = yl + 1;               // source rows of the cy = +1 / cy = -1 links
    if (BC == LB_BC_PERIODIC) {
        if (ym < 0) ym = g.ny - 1;
        if (yp >= g.ny) yp = 0;
    }
    f4a q[NF][9], r4[NF];
    uc4 mk;
#pragma unroll
    for (int i = 0; i < NF; ++i)
        gather_row<BC == LB_BC_PERIODIC ? LB_BC_PERIODIC : LB_BC_PIPE, false, false>(m.a[i], x4, yl, ym, yp, q[i], mk);
    if (BC == LB_BC_BOX) {
        const int ce = g.nx - 1 - x4;
        if (yl == 0 || yl == g.ny - 1 || x4 == 0 || (ce >= 0 && ce < 4)) {
#pragma unroll
            for (int i = 0; i < NF; ++i) row_wall(MfBox{}, m.a[i].corner, g.nx, g.ny, x4, yl, q[i]);
        }
    }
    const long long m0 = (long long)yl * g.fpitch;
    const f4a u4 = load4<false>(lane_ptr((const float *)g.u + m0, x4));
    const f4a v4 = load4<false>(lane_ptr((const float *)g.v + m0, x4));
    mf_collide_row<NF>(q, u4, v4, m, r4);
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        float *d = m.a[i].dst + (long long)yl * g.pitch;
        const long long S = g.plane;
#pragma unroll
        for (int k = 0; k < 9; ++k) store4<false>(lane_ptr(d + k * S, x4), q[i][k]);
        if (RHO) store4<false>(lane_ptr(m.a[i].rho + m0, x4), r4[i]);
    }
}

// ---- the reference's phases ----------------------------------------------------------------------------------------------------
// move_bcs (D2Q9_multifield_fisher.cl:173-289) of one field, in place behind lb_move (edge_walk, kernels_lane4.h).  The two links per
// corner that the rule skips keep what the lattice holds (lb_move has patched the corner state in).
__global__ void k_mf_move_bcs(const StepArgs a, float *f) { edge_walk(a, f, BoxEdge<MfBox>{}); }

// collide_particles (:76-124), one cell per thread: grid = (ceil(nx / 256), ny).  k_ad_collide's arithmetic with the room left by ALL
// fields in the growth term.  (cell_xy written out: the call moves the instruction text for one field.)
template <int NF>
__global__ void k_mf_collide(const MfArgs m)
{
    const StepArgs &g = m.a[0];
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= g.nx) return;
    const long long o = (long long)y * g.pitch + x, c = (long long)y * g.fpitch + x;
    float rho[NF], rho_tot = 0.f;
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        rho[i] = m.a[i].rho[c];
        rho_tot = i ? rho_tot + rho[i] : rho[i];
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        float *f = m.a[i].dst;                  // (the launcher puts the lattice relaxed in place here)
        const float *feq = m.feq[i];
        const float omega = m.a[i].omega, keep = 1.f - omega, G = m.G[i];
        const float react = (G * rho[i]) * (1.f - rho_tot);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            float v = lb_fma(f[o + k * g.plane], keep, omega * feq[o + k * g.plane]);
            if (G != 0.f) v = lb_fma(lb_w9(k), react, v);
            f[o + k * g.plane] = v;
        }
    }
}

}  // namespace
