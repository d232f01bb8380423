// kernels_multifield.h -- the kernels of coupled scalar lattices (LB_SEM_MULTIFIELD: the reference's LB_D2Q9/D2Q9_multifield_fisher.cl,
// driven as advecting_range_expansion/deterministic_fisher_waves.py:436-450 does: move + copy_buffer -> move_bcs -> update_hydro ->
// update_feq -> collide_particles, five launches and five host waits per step, each looping over the fields in every work-item).
// Included by multifield.cpp only (multifield_launch.h: what the kernels and their host code share; host.h: what the other host units see).
//   k_mf_step<BC, NF, RHO>   the fused step of NF fields: k_ad_step's plan (kernels_scalar.h) -- a lane owns four consecutive cells of
//                            a row; per field nine 16-byte loads (six displaced by one element: k_step's gather) and nine aligned
//                            16-byte stores, u and v loaded once for all fields, rho of every field when asked: 72 NF + 8 B per cell
//                            and step.  Every field's gathered populations are live before any collision -- rho_tot comes first --:
//                            36 registers per field.  The cell arithmetic is scalar_cell.h's: with one field the bits of k_ad_step.
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

namespace {

// move_bcs of D2Q9_multifield_fisher.cl for one cell (w, e, s, n: it lies in column 0 / nx-1, row 0 / ny-1); st: the eight corner
// links in the ABI's order -- f6, f8 of (0,0), f5, f7 of (nx-1,0), f5, f7 of (0,ny-1), f6, f8 of (nx-1,ny-1).  Every right-hand
// side is a post-stream value of the cell, read before anything is written, as the kernel reads f1 ... f8 first.
__device__ __forceinline__ void mf_box_cell(Cell &c, bool w, bool e, bool s, bool n, const float *st)
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

// ... for a lane's four gathered cells (x4 .. x4+3, row y).  The caller has checked that the lane holds a wall cell.
__device__ __forceinline__ void mf_box_row(const float *st, int nx, int ny, int x4, int y, f4a (&q)[9])
{
    const bool s = (y == 0), n = (y == ny - 1);
    const int ce = nx - 1 - x4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool w = (x4 == 0 && j == 0), e = (j == ce);
        if (s || n || w || e) {
            Cell c = row_cell(q, j);
            mf_box_cell(c, w, e, s, n, st);
            row_cell_put(q, j, c);
        }
    }
}

// moments of every field, rho_tot, then equilibrium, relaxation and growth of every field: a lane's four cells as two pairs, in
// place (ad_collide_row's plan, kernels_scalar.h).  A field with G = 0 skips the growth term (wave-uniform): plain relaxation.
template <int NF>
__device__ __forceinline__ void mf_collide_row(f4a (&q)[NF][9], f4a u4, f4a v4, const MfArgs &m, f4a (&r4)[NF])
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f2a ux = h ? u4.zw : u4.xy, uy = h ? v4.zw : v4.xy;
        f2a rho[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            f2a f[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) f[k] = h ? q[i][k].zw : q[i][k].xy;
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
            for (int k = 0; k < 9; ++k) f[k] = h ? q[i][k].zw : q[i][k].xy;
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

// Launch: blockDim = (64, 4), grid = (ceil(fpitch / 256), ceil(ny / 4)): a wave covers 256 cells of one row (k_ad_step's launch).
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
            for (int i = 0; i < NF; ++i) mf_box_row(m.a[i].corner, g.nx, g.ny, x4, yl, q[i]);
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
// move_bcs (D2Q9_multifield_fisher.cl:173-289) of one field, in place behind lb_move: one thread per index i, grid =
// ceil(max(nx, ny) / 256): the cells (i, 0) and (i, ny-1) of the wall rows, (0, i) and (nx-1, i) of the wall columns between them.
// The two links per corner that the rule skips keep what the lattice holds (lb_move has patched the corner state in).
__device__ __forceinline__ void mf_bcs_cell(const StepArgs &a, float *f, int x, int y)
{
    float *p = f + (long long)y * a.pitch + x;
    const long long S = a.plane;
    Cell c = {p[0], p[S], p[2 * S], p[3 * S], p[4 * S], p[5 * S], p[6 * S], p[7 * S], p[8 * S]};
    const float own[8] = {c.f6, c.f8, c.f5, c.f7, c.f5, c.f7, c.f6, c.f8};
    mf_box_cell(c, x == 0, x == a.nx - 1, y == 0, y == a.ny - 1, own);
    p[S] = c.f1; p[2 * S] = c.f2; p[3 * S] = c.f3; p[4 * S] = c.f4;
    p[5 * S] = c.f5; p[6 * S] = c.f6; p[7 * S] = c.f7; p[8 * S] = c.f8;
}

__global__ void k_mf_move_bcs(const StepArgs a, float *f)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.nx) {
        mf_bcs_cell(a, f, i, 0);
        mf_bcs_cell(a, f, i, a.ny - 1);
    }
    if (i >= 1 && i <= a.ny - 2) {
        mf_bcs_cell(a, f, 0, i);
        mf_bcs_cell(a, f, a.nx - 1, i);
    }
}

// collide_particles (:76-124), one cell per thread: grid = (ceil(nx / 256), ny).  k_ad_collide's arithmetic (kernels_scalar.h) with
// the room left by ALL fields in the growth term.
template <int NF>
__global__ void k_mf_collide(const MfArgs m)
{
    const StepArgs &g = m.a[0];
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= g.nx) return;
    const long long o = (long long)y * g.pitch + x, c = (long long)y * g.fpitch + x;
    const float w[9] = {4.f / 9.f, 1.f / 9.f, 1.f / 9.f, 1.f / 9.f, 1.f / 9.f, 1.f / 36.f, 1.f / 36.f, 1.f / 36.f, 1.f / 36.f};
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
            if (G != 0.f) v = lb_fma(w[k], react, v);
            f[o + k * g.plane] = v;
        }
    }
}

}  // namespace
