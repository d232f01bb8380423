// kernels_advected.h -- a flow and the scalars it carries, one launch per step.  Included by advected.cpp only (advected_launch.h: what
// the kernel and its host code share; host.h: what the other host units see).
//
// One periodic flow lattice (LB_SEM_OPENCL, no obstacles) and NS = 1 ... 2 scalar lattices (LB_SEM_DIFFUSION, LB_BC_PERIODIC) of the same
// box.  After streaming the step of the pair is local to the cell: the flow's collision forms rho, u, v of the cell from its gathered
// populations BEFORE it relaxes them, and the scalar's collision needs exactly those u, v.
//   k_fa_step<NS, REACT, LAST>   on the lane-of-four plan (kernels_lane4.h): gathers the flow's nine planes and nine per scalar, collides
//                                the flow (k_step's gather_row and collide_row<LB_BC_PERIODIC, false>: its bits), hands u4, v4 on in
//                                registers, collides each scalar (scalar_cell.h's cell, k_ad_step's bits; REACT: a member with G != 0
//                                takes the growth term, one with G == 0 the plain cell -- a wave-uniform branch, no instantiation per
//                                member), 9 (1 + NS) aligned 16-byte stores.  LAST (a call's last launch): the flow's rho, u, v, and each
//                                scalar's rho and the same u, v into the scalar's own planes.  72 (1 + NS) B per cell and step.
// The velocity of step t is the one the flow's step t forms from its STREAMED populations -- what k_step<..., MACRO = true> stores --, not
// the one rebuilt from the post-collision populations, which differs by rounding (include/lb_hip.h, LB_FLAG_EAGER_MACRO).
// The 1 + NS launch form of the same step (k_step<MACRO> then one k_ad_step per scalar reading the flow's u, v planes: advected.cpp) is
// held to this kernel bitwise.
#pragma once
#include "scalar_cell.h"
#include "advected_launch.h"
#include "kernels_lane4.h"      // lane_gather, pair_of, store_planes

namespace {

// moments, equilibrium, relaxation [, growth] of a lane's four gathered cells of one scalar as two pairs, in place: the statements of
// kernels_scalar.h's ad_collide_row written out -- that header emits the scalar lattice's plain kernels and belongs to scalar.cpp
// alone --, the arithmetic itself is scalar_cell.h's, as in kernels_nutrient.h
template <bool REACT>
__device__ __forceinline__ void fa_scalar_row(f4a (&q)[9], f4a u4, f4a v4, float omega, float G, f4a &r4)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f2a f[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = pair_of(q[k], h);
        const f2a ux = pair_of(u4, h), uy = pair_of(v4, h);
        const f2a rho = ad_rho_t<f2a>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]);
        ad_relax_t<f2a, REACT>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], omega, G, rho, ux, uy);
        if (h) r4.zw = rho;
        else r4.xy = rho;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (h) q[k].zw = f[k];
            else q[k].xy = f[k];
        }
    }
}

// Launch: blockDim = (64, 4), grid = (ceil(fpitch / 256), ceil(ny / 4)) -- k_ad_step's.  Every gather is issued before the first
// collision: the loads of all 1 + NS lattices are in flight together.
template <int NS, bool REACT, bool LAST>
__global__ __launch_bounds__(256) void k_fa_step(const FaArgs m)
{
    const StepArgs &g = m.flow;                 // the set's geometry
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int yl = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);
    if (x4 >= g.fpitch || yl >= g.ny) return;
    int ym = yl - 1, yp = yl + 1;               // source rows of the cy = +1 / cy = -1 links
    if (ym < 0) ym = g.ny - 1;
    if (yp >= g.ny) yp = 0;
    f4a q[9], c[NS][9], r4, u4, v4, cr[NS];
    uc4 mk;
    gather_row<LB_BC_PERIODIC, false, false>(g, x4, yl, ym, yp, q, mk);
#pragma unroll
    for (int i = 0; i < NS; ++i) lane_gather<LB_BC_PERIODIC>(m.s[i], x4, yl, ym, yp, c[i]);
    collide_row<LB_BC_PERIODIC, false>(g, x4, yl, q, mk, r4, u4, v4);
    store_planes(g, yl, x4, q);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        if (REACT && m.G[i] != 0.f) fa_scalar_row<true>(c[i], u4, v4, m.s[i].omega, m.G[i], cr[i]);
        else fa_scalar_row<false>(c[i], u4, v4, m.s[i].omega, 0.f, cr[i]);
        store_planes(m.s[i], yl, x4, c[i]);
    }
    if (LAST) {
        const long long m0 = (long long)yl * g.fpitch;
        store_moments(g, m0, x4, r4, u4, v4);
#pragma unroll
        for (int i = 0; i < NS; ++i) store_moments(m.s[i], m0, x4, cr[i], u4, v4);
    }
}

}  // namespace
