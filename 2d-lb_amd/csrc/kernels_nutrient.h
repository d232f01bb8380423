// kernels_nutrient.h -- the kernels of a population and the nutrient it eats under a velocity solved from the population (the
// reference's LB_D2Q9/reaction_diffusion/surfactant_nutrient_waves.cl, driven as surfactant_nutrient_waves.py's run does:
// move_periodic -> copy -> update_hydro -> the spectral solve -> [update_psi -> update_pseudo_force] -> update_feq ->
// collide_particles[_attraction], some 25 launches and array passes per step with a host wait behind each).  Included by nutrient.cpp
// only (nutrient_launch.h: what the kernels and their host code share; host.h: what the other host units see).
//
// Two scalar lattices (LB_SEM_DIFFUSION, LB_BC_PERIODIC) in one box, the population p and the nutrient n.  The velocity is not local:
// it comes from the spectral solve over rho_p after streaming, which k_ad_moments stores and three launches turn into u, v of the
// population's handle (spectral.cpp).  What is left of the step is local to the cell -- and, CLUMPY, to its eight neighbours' psi:
//   k_sn_step<CLUMPY, LAST>      on the lane-of-four plan (kernels_lane4.h): gathers both lattices, both densities from the gathered
//                                links, one load each of u and v for both, scalar_cell.h's relaxation (k_ad_step's bits), +- w_k G rho_p
//                                rho_n, stores.  CLUMPY: psi of the stored rho_p plane of the workgroup's SN_ROWS rows, one halo row
//                                above and below and one halo cell left and right in LDS (wrap on the INDEX, LANE4_LDS_ROW's layout),
//                                F = -cs^2 G_chen psi sum_k w_k c_k psi(x + c_k), + (w_k c_k.F) / cs^2 on the population.  LAST (a
//                                run's last step): rho_n, u, v into the nutrient member; CLUMPY: psi, Fx, Fy as well (rho_p is in
//                                memory already: k_ad_moments' store, the same bits).  144 B + 8 B (CLUMPY: + 6 B) per cell and step.
//   k_sn_forces, k_sn_collide<CLUMPY>   the reference's stages one by one, one cell per thread (move, update_hydro and update_feq are
//                                the scalar lattice's k_move, k_ad_hydro and k_ad_feq).  They keep the un-fused order -- feq stored,
//                                then f (1 - omega) + omega feq -- and so round differently from the fused cell, where omega enters
//                                through rho: held to it by the contract's tolerance, as k_ad_collide is to k_ad_step.
// There is no floor at zero (the colonies of kernels_rocket.h have one).
#pragma once
#include "scalar_cell.h"
#include "multifluid_cell.h"    // mc_stencil_t, mc_psi
#include "nutrient_launch.h"
#include "kernels_lane4.h"

namespace {

__device__ __forceinline__ float sn_psi(const SnArgs &m, float rho_p) { return mc_psi(LB_PSI_SHAN_CHEN, m.rho_o, rho_p); }

// F = kf (psi(x) S), S the stencil sum over psi; p[row][col] with row 0 = y - 1, col 0 = x - 1
template <typename T>
__device__ __forceinline__ void sn_force_t(const SnArgs &m, const T (&p)[3][3], T &Fx, T &Fy)
{
    T sx, sy;
    mc_stencil_t<T>(p, sx, sy);
    const T kf = lb_splat<T>(m.kf);
    const T px = p[1][1] * sx;
    const T py = p[1][1] * sy;
    Fx = kf * px;
    Fy = kf * py;
}

// f_k += (w_k c_k.F) / cs^2, k = 1 ... 8
template <typename T>
__device__ __forceinline__ void sn_push_t(const SnArgs &m, T (&f)[9], T Fx, T Fy)
{
    const T inv = lb_splat<T>(m.inv_cs2), w1 = lb_splat<T>(1.f / 9.f), w2 = lb_splat<T>(1.f / 36.f);
    const T pp = Fx + Fy, pm = Fx - Fy;
    const T cF[9] = {pp, Fx, Fy, -Fx, -Fy, pp, -pm, -pp, pm};      // c_k.F (cF[0] is not used)
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        const T t = (k < 5 ? w1 : w2) * cF[k];
        f[k] = lb_fma(t, inv, f[k]);
    }
}

// Stages 2, 5 and 6 of a lane's four cells of row yl for both lattices, and the stores: q = the gathered populations, np = psi
// around the cells (lane_nb_load's layout; CLUMPY only)
template <bool CLUMPY, bool LAST>
__device__ __forceinline__ void sn_collide_lane(const SnArgs &m, int x4, int yl, f4a (&q)[2][9], const float (&np)[3][6])
{
    const long long m0 = (long long)yl * m.a[0].fpitch;
    const f4a u4 = load4<false>(lane_ptr((const float *)m.a[0].u + m0, x4));
    const f4a v4 = load4<false>(lane_ptr((const float *)m.a[0].v + m0, x4));
    f4a rn4, Fx4, Fy4, ps4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f2a fp[9], fn[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            fp[k] = pair_of(q[0][k], h);
            fn[k] = pair_of(q[1][k], h);
        }
        const f2a ux = pair_of(u4, h), uy = pair_of(v4, h);
        const f2a rho_p = ad_rho_t<f2a>(fp[0], fp[1], fp[2], fp[3], fp[4], fp[5], fp[6], fp[7], fp[8]);
        const f2a rho_n = ad_rho_t<f2a>(fn[0], fn[1], fn[2], fn[3], fn[4], fn[5], fn[6], fn[7], fn[8]);
        ad_relax_t<f2a, false>(fp[0], fp[1], fp[2], fp[3], fp[4], fp[5], fp[6], fp[7], fp[8], m.a[0].omega, 0.f, rho_p, ux, uy);
        ad_relax_t<f2a, false>(fn[0], fn[1], fn[2], fn[3], fn[4], fn[5], fn[6], fn[7], fn[8], m.a[1].omega, 0.f, rho_n, ux, uy);
        // + w_k ((G rho_p) rho_n) and - w_k (...): ad_grow_t with the nutrient for the room, the same product negated exactly
        ad_grow_t<f2a>(fp[0], fp[1], fp[2], fp[3], fp[4], fp[5], fp[6], fp[7], fp[8], m.G, rho_p, rho_n);
        ad_grow_t<f2a>(fn[0], fn[1], fn[2], fn[3], fn[4], fn[5], fn[6], fn[7], fn[8], -m.G, rho_p, rho_n);
        if (CLUMPY) {
            f2a p[3][3], Fx, Fy;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) p[r][c] = f2a{np[r][2 * h + c], np[r][2 * h + c + 1]};
            sn_force_t<f2a>(m, p, Fx, Fy);
            sn_push_t<f2a>(m, fp, Fx, Fy);
            if (h) { Fx4.zw = Fx; Fy4.zw = Fy; ps4.zw = p[1][1]; }
            else { Fx4.xy = Fx; Fy4.xy = Fy; ps4.xy = p[1][1]; }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (h) { q[0][k].zw = fp[k]; q[1][k].zw = fn[k]; }
            else { q[0][k].xy = fp[k]; q[1][k].xy = fn[k]; }
        }
        if (h) rn4.zw = rho_n;
        else rn4.xy = rho_n;
    }
    store_planes(m.a[0], yl, x4, q[0]);
    store_planes(m.a[1], yl, x4, q[1]);
    if (LAST) {
        store4<false>(lane_ptr(m.a[1].rho + m0, x4), rn4);
        store4<false>(lane_ptr(m.a[1].u + m0, x4), u4);
        store4<false>(lane_ptr(m.a[1].v + m0, x4), v4);
        if (CLUMPY) {
            store4<false>(lane_ptr(m.psi + m0, x4), ps4);
            store4<false>(lane_ptr(m.Fx + m0, x4), Fx4);
            store4<false>(lane_ptr(m.Fy + m0, x4), Fy4);
        }
    }
}

// Launch: blockDim = (64, SN_ROWS), grid = (ceil(fpitch / 256), ceil(ny / SN_ROWS)).  CLUMPY: LDS row r holds psi of the box row
// y0 - 1 + r, wrapped: wave w fills row w + 1 (its own), wave 0 the halo row 0 and wave 1 the halo row SN_ROWS + 1 as well; lanes 0
// and 1 add the halo columns behind the row's own writes.  Nobody leaves before the barrier.
template <bool CLUMPY, bool LAST>
__global__ __launch_bounds__(64 * SN_ROWS) void k_sn_step(const SnArgs m)
{
    __shared__ __attribute__((aligned(16))) float lds[CLUMPY ? SN_ROWS + 2 : 1][CLUMPY ? LANE4_LDS_ROW : 4];
    const StepArgs &a0 = m.a[0];
    const int lane = threadIdx.x, w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int x0 = blockIdx.x * 256, x4 = x0 + lane * 4;
    const int y0 = blockIdx.y * SN_ROWS, yl = y0 + w;
    if (CLUMPY) {
        const int inside = min(256, a0.nx - x0);            // cells of the tile inside the box (<= 0: a tile of row padding)
        int xw = x0 - 1, xe = x0 + inside;
        if (xw < 0) xw = a0.nx - 1;
        if (xe >= a0.nx) xe = 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (t == 1 && w > 1) break;
            const int r = t == 0 ? w + 1 : (w == 0 ? 0 : SN_ROWS + 1);
            int y = y0 - 1 + r;                              // ... as a row of the box
            if (y < 0) y = a0.ny - 1;
            if (y >= a0.ny) y -= a0.ny;
            y = min(max(y, 0), a0.ny - 1);                  // (rows past the halo of the last workgroup: in the box, never used)
            const float *row = a0.rho + (long long)y * a0.fpitch;
            if (x4 < a0.fpitch) {
                const f4a d = load4<false>(lane_ptr(row, x4));
                f4a ps;
#pragma unroll
                for (int j = 0; j < 4; ++j) ps[j] = sn_psi(m, d[j]);
                *reinterpret_cast<f4a *>(&lds[r][4 + lane * 4]) = ps;
            }
            if (inside > 0 && lane < 2) {
                // (behind the row's own writes: the east halo takes the slot of the first padding cell, and a wave's LDS writes land in order)
                lds[r][lane ? 4 + inside : 3] = sn_psi(m, row[lane ? xe : xw]);
            }
        }
        __syncthreads();
    }
    if (x4 >= a0.fpitch || yl >= a0.ny) return;
    int ym = yl - 1, yp = yl + 1;
    if (ym < 0) ym = a0.ny - 1;
    if (yp >= a0.ny) yp = 0;
    f4a q[2][9];
    lane_gather<LB_BC_PERIODIC>(m.a[0], x4, yl, ym, yp, q[0]);
    lane_gather<LB_BC_PERIODIC>(m.a[1], x4, yl, ym, yp, q[1]);
    float np[3][6] = {};
    if (CLUMPY) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float *rp = &lds[w + r][4 + lane * 4];
            const f4a vp = *reinterpret_cast<const f4a *>(rp);
            np[r][0] = rp[-1]; np[r][1] = vp.x; np[r][2] = vp.y; np[r][3] = vp.z; np[r][4] = vp.w; np[r][5] = rp[4];
        }
    }
    sn_collide_lane<CLUMPY, LAST>(m, x4, yl, q, np);
}

// ---- the reference's stages, one cell per thread: grid = (ceil(nx / 256), ny) ----------------------------------------------------
// update_psi + update_pseudo_force, from the stored rho_p
__global__ void k_sn_forces(const SnArgs m)
{
    const StepArgs &a = m.a[0];
    int x, y;
    if (!cell_xy(a, x, y)) return;
    float p[3][3], Fx, Fy;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int yy = y - 1 + r, xx = x - 1 + c;
            yy = yy < 0 ? a.ny - 1 : (yy >= a.ny ? 0 : yy);
            xx = xx < 0 ? a.nx - 1 : (xx >= a.nx ? 0 : xx);
            p[r][c] = sn_psi(m, a.rho[(long long)yy * a.fpitch + xx]);
        }
    sn_force_t<float>(m, p, Fx, Fy);
    const long long o = (long long)y * a.fpitch + x;
    m.psi[o] = p[1][1];
    m.Fx[o] = Fx;
    m.Fy[o] = Fy;
}

// collide_particles / collide_particles_attraction: both lattices at a[i].dst (the launcher puts the current lattice there) relaxed
// in place towards the stored feq, from the stored densities and F
template <bool CLUMPY>
__global__ void k_sn_collide(const SnArgs m, const float *feq_p, const float *feq_n)
{
    const StepArgs &a = m.a[0];
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long o = (long long)y * a.pitch + x, c = (long long)y * a.fpitch + x, S = a.plane;
    float *fp = m.a[0].dst + o, *fn = m.a[1].dst + o;
    const float rho_p = m.a[0].rho[c], rho_n = m.a[1].rho[c];
    float f[9];
    {
        const float keep = 1.f - m.a[0].omega;
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = lb_fma(fp[k * S], keep, m.a[0].omega * feq_p[o + k * S]);
        ad_grow_t<float>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], m.G, rho_p, rho_n);
        if (CLUMPY) sn_push_t<float>(m, f, m.Fx[c], m.Fy[c]);
#pragma unroll
        for (int k = 0; k < 9; ++k) fp[k * S] = f[k];
    }
    {
        const float keep = 1.f - m.a[1].omega;
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = lb_fma(fn[k * S], keep, m.a[1].omega * feq_n[o + k * S]);
        ad_grow_t<float>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], -m.G, rho_p, rho_n);
#pragma unroll
        for (int k = 0; k < 9; ++k) fn[k * S] = f[k];
    }
}

}  // namespace
