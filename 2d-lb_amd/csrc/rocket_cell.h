// rocket_cell.h -- device-side arithmetic of one cell of a surfactant-propelled colony (LB_SEM_ROCKET): the reference's
// LB_D2Q9/rocket_yeast/rocket_yeast.cl (LB_ROCKET_FLOW: update_u_and_v, update_psi, update_pseudo_force, update_feq,
// collide_particles) and rocket_yeast_forces_only.cl (LB_ROCKET_FORCES: update_surf_tension, update_surface_forces,
// update_pressure_force, update_u_and_v, update_feq, collide_particles).  Written once for a scalar cell (T = float: the stage
// kernels) and for a pair of x-adjacent cells (T = f2a: the fused kernels), in the manner of multifluid_cell.h: the same operations in
// the same order, every multiply-add an explicit lb_fma and every other statement ONE operation, so a cell gets the same bits
// whichever kernel computes it -- the one-launch step, the two-launch step and the stages are held to each other BITWISE.  What
// crosses a stage boundary (rho, u, v, psi / S, the forces, feq_k) is a float32 of its own in all of them.
//
// float32 throughout.  The stencil is multifluid_cell.h's (mc_stencil_t: the links in the reference's order); the equilibrium is the
// scalar lattice's (scalar_cell.h's ad_feq_cell, the constant 3 for 1 / cs^2: the stage is k_ad_feq itself); the velocity and the
// forces take float32(1. / (cs * cs)) of the float32 cs, as the reference's kernels form it (RyArgs::inv_cs2).  expf and powf are
// the library's.  The pseudopotential and the surface coverage are functions of one density: evaluated once per density read.
#pragma once
#include "scalar_cell.h"
#include "multifluid_cell.h"    // mc_stencil_t, mc_psi
#include "rocket_launch.h"

namespace {

// S(c) = pow(1 - exp(-max(c, 0) / c_o), alpha)            rocket_yeast_forces_only.cl: update_surf_tension
__device__ __forceinline__ float ry_surf(float c_o, float alpha, float rho)
{
    const float r = rho < 0.f ? 0.f : rho;
    const float q = r / c_o;
    const float ex = expf(-q);
    const float d = 1.f - ex;
    return powf(d, alpha);
}

// the two stencil operands from the two densities: A from the surfactant's, B from the population's
template <int MODE>
__device__ __forceinline__ float ry_op_a(const RyArgs &m, float rho_c) { return MODE == LB_ROCKET_FLOW ? rho_c : ry_surf(m.c_o, m.alpha, rho_c); }
template <int MODE>
__device__ __forceinline__ float ry_op_b(const RyArgs &m, float rho_p) { return MODE == LB_ROCKET_FLOW ? mc_psi(LB_PSI_SHAN_CHEN, m.rho_o, rho_p) : rho_p; }

__device__ __forceinline__ float ry_floor0(float x) { return x < 0.f ? 0.f : x; }       // (NaN stays, as the reference's comparison leaves it)
__device__ __forceinline__ f2a ry_floor0(f2a x) { return f2a{x.x < 0.f ? 0.f : x.x, x.y < 0.f ? 0.f : x.y}; }
// rho > 1 ? 0 : g
__device__ __forceinline__ float ry_room(float rho, float g) { return rho > 1.f ? 0.f : g; }
__device__ __forceinline__ f2a ry_room(f2a rho, f2a g) { return f2a{rho.x > 1.f ? 0.f : g.x, rho.y > 1.f ? 0.f : g.y}; }

// Stage 3, one stencil times (-epsilon / cs^2): FLOW's velocity (over rho_c), FORCES' surface force (over S)
template <typename T>
__device__ __forceinline__ void ry_marangoni_t(const RyArgs &m, const T (&p)[3][3], T &x, T &y)
{
    T sx, sy;
    mc_stencil_t<T>(p, sx, sy);
    const T ke = lb_splat<T>(m.ke);
    x = ke * sx;
    y = ke * sy;
}

// FLOW: F = (-G_chen psi(x)) grad_w psi
template <typename T>
__device__ __forceinline__ void ry_pseudo_force_t(const RyArgs &m, const T (&p)[3][3], T &Fx, T &Fy)
{
    T sx, sy;
    mc_stencil_t<T>(p, sx, sy);
    const T c = lb_splat<T>(m.ngc) * p[1][1];
    Fx = c * sx;
    Fy = c * sy;
}

// FORCES: F_p = (-G_chen (grad_w rho_p / cs^2)) (rho_p - rho_o)
template <typename T>
__device__ __forceinline__ void ry_pressure_force_t(const RyArgs &m, const T (&p)[3][3], T &Fx, T &Fy)
{
    T sx, sy;
    mc_stencil_t<T>(p, sx, sy);
    const T inv = lb_splat<T>(m.inv_cs2);
    const T gx = sx * inv;
    const T gy = sy * inv;
    const T d = p[1][1] - lb_splat<T>(m.rho_o);
    const T cx = lb_splat<T>(m.ngc) * gx;
    const T cy = lb_splat<T>(m.ngc) * gy;
    Fx = cx * d;
    Fy = cy * d;
}

// Stage 4: ad_feq_cell (scalar_cell.h) for T
template <typename T>
__device__ __forceinline__ void ry_feq_t(T (&e)[9], T rho, T ux, T uy)
{
    const T r0 = (4.f / 9.f) * rho, r1 = (1.f / 9.f) * rho, r2 = (1.f / 36.f) * rho;
    const T r13 = 3.f * r1, r23 = 3.f * r2;
    e[0] = r0;
    ad_feq_pair<T>(r1, r13, ux, e[1], e[3]);
    ad_feq_pair<T>(r1, r13, uy, e[2], e[4]);
    ad_feq_pair<T>(r2, r23, ux + uy, e[5], e[7]);
    ad_feq_pair<T>(r2, r23, ux - uy, e[8], e[6]);
}

// Stage 5, the population: max(0, f_k (1 - omega) + omega feq_k + w_k G rho (1 - rho) [FLOW: + (w_k c_k.F) / cs^2]); FORCES: no
// growth where rho > 1
template <typename T, int MODE>
__device__ __forceinline__ void ry_relax_pop_t(const RyArgs &m, T (&f)[9], const T (&e)[9], float omega, T rho, T Fx, T Fy)
{
    const T keep = lb_splat<T>(1.f - omega), om = lb_splat<T>(omega), inv = lb_splat<T>(m.inv_cs2);
    const T w[9] = {lb_splat<T>(4.f / 9.f), lb_splat<T>(1.f / 9.f), lb_splat<T>(1.f / 9.f), lb_splat<T>(1.f / 9.f), lb_splat<T>(1.f / 9.f),
                    lb_splat<T>(1.f / 36.f), lb_splat<T>(1.f / 36.f), lb_splat<T>(1.f / 36.f), lb_splat<T>(1.f / 36.f)};
    const T gr = lb_splat<T>(m.G) * rho;
    const T room = lb_splat<T>(1.f) - rho;
    T g = gr * room;
    if (MODE == LB_ROCKET_FORCES) g = ry_room(rho, g);
    const T pp = Fx + Fy, pm = Fx - Fy;
    const T cF[9] = {pp, Fx, Fy, -Fx, -Fy, pp, -pm, -pp, pm};      // c_k.F (cF[0] is not used)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        T v = lb_fma(f[k], keep, om * e[k]);
        v = lb_fma(w[k], g, v);
        if (MODE == LB_ROCKET_FLOW && k > 0) {
            const T t = w[k] * cF[k];
            v = lb_fma(t, inv, v);
        }
        f[k] = ry_floor0(v);
    }
}

// ... and the surfactant: f_k (1 - omega_c) + omega_c feq_k + w_k G_c rho_p
template <typename T>
__device__ __forceinline__ void ry_relax_surf_t(const RyArgs &m, T (&f)[9], const T (&e)[9], float omega, T rho_p)
{
    const T keep = lb_splat<T>(1.f - omega), om = lb_splat<T>(omega);
    const T w[9] = {lb_splat<T>(4.f / 9.f), lb_splat<T>(1.f / 9.f), lb_splat<T>(1.f / 9.f), lb_splat<T>(1.f / 9.f), lb_splat<T>(1.f / 9.f),
                    lb_splat<T>(1.f / 36.f), lb_splat<T>(1.f / 36.f), lb_splat<T>(1.f / 36.f), lb_splat<T>(1.f / 36.f)};
    const T g = lb_splat<T>(m.Gc) * rho_p;
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = lb_fma(w[k], g, lb_fma(f[k], keep, om * e[k]));
}

}  // namespace
