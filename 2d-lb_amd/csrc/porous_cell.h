// porous_cell.h -- device-side arithmetic of one cell of forced flow in a porous medium (LB_SEM_POROUS): the reference's
// LB_D2Q9/porous_media/single_component.cl -- update_hydro_pourous :214-274, update_forces_pourous :276-335, update_bary_velocity
// :161-212, update_feq_pourous :11-63, collide_particles_pourous :65-118.  Written once for a scalar cell (T = float: the phase
// kernels) and for a pair of x-adjacent cells (T = f2a: the fused kernel), in the style of d2q9_cell.h and scalar_cell.h: the same
// operations in the same order, every multiply-add an explicit lb_fma and every other statement ONE operation, so a cell gets the same
// bits whichever form, and whichever kernel, computes it -- the fused step and the eight phases are held to each other BITWISE.  What
// crosses a phase boundary (rho, u, v, G, u_b, feq_k) is a float32 of its own in both: stored by the phases, a register of the fused
// cell.
//
// float32 throughout (the reference's fork computes in float64).  1 / cs^2 is the constant 3; the divisions by epsilon are
// multiplications by float32 constants formed once on the host (PmExtra); the divisions by rho, K and sqrt(K) and the square root are
// IEEE (hipcc's default: correctly rounded; no approximate reciprocal here).
#pragma once
#include "d2q9_cell.h"
#include "porous_launch.h"

namespace {

constexpr float PM_ZERO_DENSITY = 1e-6f;        // single_component.cl:9

__device__ __forceinline__ float pm_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ f2a pm_sqrt(f2a x) { return f2a{__builtin_sqrtf(x.x), __builtin_sqrtf(x.y)}; }
// dense ? a : 0, per cell
__device__ __forceinline__ float pm_if_dense(float rho, float a) { return rho > PM_ZERO_DENSITY ? a : 0.f; }
__device__ __forceinline__ f2a pm_if_dense(f2a rho, f2a a)
{
    return f2a{rho.x > PM_ZERO_DENSITY ? a.x : 0.f, rho.y > PM_ZERO_DENSITY ? a.y : 0.f};
}

// Stage 3.  rho = sum f, left to right; mx, my = sum f c in the order of the links (a link with c = 0 adds an exact 0 there): the
// sums update_bary_velocity forms again from the same f; u, v = mx / rho, my / rho where rho > 1e-6, else 0.
template <typename T>
__device__ __forceinline__ void pm_hydro_t(const T (&f)[9], T &rho, T &mx, T &my, T &u, T &v)
{
    rho = f[0] + f[1] + f[2] + f[3] + f[4] + f[5] + f[6] + f[7] + f[8];
    mx = f[1] - f[3] + f[5] - f[6] - f[7] + f[8];
    my = f[2] - f[4] + f[5] + f[6] - f[7] - f[8];
    const T qu = mx / rho, qv = my / rho;
    u = pm_if_dense(rho, qu);
    v = pm_if_dense(rho, qv);
}

// Stages 4 and 5 for one component: g0 = the body force of the cell (constant [+ field]), w = that component of the velocity of
// stage 3, mag = |u|.  G = ((epsilon g0) - ((epsilon nu) w) / K) - (((epsilon Fe) mag) w) / sqrt(K), 0 where rho <= 1e-6.
template <typename T>
__device__ __forceinline__ T pm_force_t(const PmExtra &e, T rho, T g0, T w, T mag)
{
    const T a = lb_splat<T>(e.eps) * g0;
    const T lin = lb_splat<T>(e.en) * w;
    const T b = lin / lb_splat<T>(e.K);
    const T quad0 = lb_splat<T>(e.ef) * mag;
    const T quad = quad0 * w;
    const T c = quad / lb_splat<T>(e.sqrtK);
    const T ab = a - b;
    const T g = ab - c;
    return pm_if_dense(rho, g);
}

template <typename T>
__device__ __forceinline__ T pm_speed_t(T u, T v)
{
    const T vv = v * v;
    return pm_sqrt(lb_fma(u, u, vv));
}

// Stage 6 for one component: (m + (rho G) / 2) / rho.  rho = 0: NaN, as the reference.
template <typename T>
__device__ __forceinline__ T pm_bary_t(T rho, T m, T G)
{
    const T rg = rho * G;
    const T s = lb_fma(lb_splat<T>(0.5f), rg, m);
    return s / rho;
}

// Stage 7.  feq_k = (w_k rho) (base + (4.5 / eps) cu^2 +- 3 cu), base = 1 - (1.5 / eps) u_b^2.
template <typename T>
__device__ __forceinline__ void pm_feq_pair(const PmExtra &e, T r, T base, T cu, T &fp, T &fm)
{
    const T q = lb_splat<T>(e.a45) * cu;
    const T t = lb_fma(q, cu, base);
    const T ip = lb_fma(lb_splat<T>(3.f), cu, t);
    const T im = lb_fma(lb_splat<T>(-3.f), cu, t);
    fp = r * ip;
    fm = r * im;
}

template <typename T>
__device__ __forceinline__ void pm_feq_t(const PmExtra &e, T (&q)[9], T rho, T ub, T vb)
{
    const T r0 = (4.f / 9.f) * rho, r1 = (1.f / 9.f) * rho, r2 = (1.f / 36.f) * rho;
    const T vv = vb * vb;
    const T usq = lb_fma(ub, ub, vv);
    const T base = lb_fma(lb_splat<T>(-e.a15), usq, lb_splat<T>(1.f));
    const T dp = ub + vb, dm = ub - vb;
    q[0] = r0 * base;
    pm_feq_pair<T>(e, r1, base, ub, q[1], q[3]);
    pm_feq_pair<T>(e, r1, base, vb, q[2], q[4]);
    pm_feq_pair<T>(e, r2, base, dp, q[5], q[7]);
    pm_feq_pair<T>(e, r2, base, dm, q[8], q[6]);
}

// Stage 8.  f_k := fma(w_k s, inner_k, fma(f_k, 1 - omega, omega feq_k)), s = rho (1 - omega / 2),
// inner_k = base + (9 / eps) cG cu +- 3 cG, base = -(3 / eps) u_b.G.
template <typename T>
__device__ __forceinline__ void pm_relax_pair(const PmExtra &e, T keep, T om, T ws, T base, T cG, T cu, T &fp, T &fm, T ep, T em)
{
    const T q = lb_splat<T>(e.b9) * cG;
    const T t = lb_fma(q, cu, base);
    const T ip = lb_fma(lb_splat<T>(3.f), cG, t);
    const T im = lb_fma(lb_splat<T>(-3.f), cG, t);
    const T op = om * ep, omm = om * em;
    const T rp = lb_fma(fp, keep, op);
    const T rm = lb_fma(fm, keep, omm);
    fp = lb_fma(ws, ip, rp);
    fm = lb_fma(ws, im, rm);
}

template <typename T>
__device__ __forceinline__ void pm_relax_t(const PmExtra &e, T (&f)[9], const T (&q)[9], float omega, T rho, T ub, T vb, T Gx, T Gy)
{
    const T keep = lb_splat<T>(1.f - omega), om = lb_splat<T>(omega);
    const T s = rho * lb_splat<T>(e.hw);
    const T s0 = (4.f / 9.f) * s, s1 = (1.f / 9.f) * s, s2 = (1.f / 36.f) * s;
    const T gv = Gy * vb;
    const T uG = lb_fma(Gx, ub, gv);
    const T base = lb_splat<T>(-e.b3) * uG;
    const T o0 = om * q[0];
    const T r0 = lb_fma(f[0], keep, o0);
    f[0] = lb_fma(s0, base, r0);
    const T up = ub + vb, um = ub - vb, Gp = Gx + Gy, Gm = Gx - Gy;
    pm_relax_pair<T>(e, keep, om, s1, base, Gx, ub, f[1], f[3], q[1], q[3]);
    pm_relax_pair<T>(e, keep, om, s1, base, Gy, vb, f[2], f[4], q[2], q[4]);
    pm_relax_pair<T>(e, keep, om, s2, base, Gp, up, f[5], f[7], q[5], q[7]);
    pm_relax_pair<T>(e, keep, om, s2, base, Gm, um, f[8], f[6], q[8], q[6]);
}

}  // namespace
