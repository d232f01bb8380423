// multifluid_cell.h -- device-side arithmetic of one cell of a set of Shan-Chen fluids (LB_SEM_MULTIFLUID): the reference's
// LB_D2Q9/multicomponent_multiphase/multi.cl -- update_hydro_fluid :275-328, add_constant_g_force :541-566, add_interaction_force
// :667-791 with get_psi :608-643, update_bary_velocity :222-273, update_feq_fluid :11-75, collide_particles_fluid :77-131,
// add_eating_collision :133-180, add_growth :182-220.  Written once for a scalar cell (T = float: the phase kernels) and for a pair
// of x-adjacent cells (T = f2a: the fused kernels), in the manner of porous_cell.h: the same operations in the same order, every
// multiply-add an explicit lb_fma and every other statement ONE operation, so a cell gets the same bits whichever kernel computes
// it -- the two-launch step and the phases are held to each other BITWISE.  What crosses a phase boundary (rho, u, v, G, u_b, feq_k)
// is a float32 of its own in both.
//
// float32 throughout (the reference computes in float64).  1 / cs^2 is the constant 3; the sums run in the reference's link and fluid
// order; the divisions are IEEE; expf and powf are the library's, not the fast intrinsics.  The pseudopotential is a function of one
// density: it is evaluated once per density read (mc_psi, a float), never per link as the reference does.
//
// The equilibrium and the relaxation are porous_cell.h's at epsilon = 1 (pm_feq_t; pm_relax_t with rho := 1, because G is a FORCE
// here and a force per density there): the scalars of PmExtra are then the exact constants 1.5, 4.5, 3, 9, and the product by 1 is exact.
#pragma once
#include "porous_cell.h"
#include "multifluid_launch.h"

namespace {

constexpr float MC_ZERO_DENSITY = 1e-12f;       // multi.cl:9

__device__ __forceinline__ float mc_if_dense(float rho, float a) { return rho > MC_ZERO_DENSITY ? a : 0.f; }
__device__ __forceinline__ f2a mc_if_dense(f2a rho, f2a a)
{
    return f2a{rho.x > MC_ZERO_DENSITY ? a.x : 0.f, rho.y > MC_ZERO_DENSITY ? a.y : 0.f};
}
__device__ __forceinline__ float mc_abs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ f2a mc_abs(f2a x) { return f2a{__builtin_fabsf(x.x), __builtin_fabsf(x.y)}; }
// a < b ? c : 0, per cell (false for NaN, as the reference's comparison)
__device__ __forceinline__ float mc_if_less(float a, float b, float c) { return a < b ? c : 0.f; }
__device__ __forceinline__ f2a mc_if_less(f2a a, f2a b, f2a c) { return f2a{a.x < b.x ? c.x : 0.f, a.y < b.y ? c.y : 0.f}; }
// lo < r && r < hi ? c : 0, per cell
__device__ __forceinline__ float mc_if_inside(float r, float lo, float hi, float c) { return (r > lo && r < hi) ? c : 0.f; }
__device__ __forceinline__ f2a mc_if_inside(f2a r, float lo, float hi, float c)
{
    return f2a{(r.x > lo && r.x < hi) ? c : 0.f, (r.y > lo && r.y < hi) ? c : 0.f};
}

// Stage 2.  rho = sum f, left to right; mx, my = sum f c in the order of the links; u, v = mx / rho, my / rho where rho > 1e-12.
template <typename T>
__device__ __forceinline__ void mc_hydro_t(const T (&f)[9], T &rho, T &mx, T &my, T &u, T &v)
{
    rho = f[0] + f[1] + f[2] + f[3] + f[4] + f[5] + f[6] + f[7] + f[8];
    mx = f[1] - f[3] + f[5] - f[6] - f[7] + f[8];
    my = f[2] - f[4] + f[5] + f[6] - f[7] - f[8];
    const T qu = mx / rho, qv = my / rho;
    u = mc_if_dense(rho, qu);
    v = mc_if_dense(rho, qv);
}

// get_psi for one density.  potential is uniform over the launch.
__device__ __forceinline__ float mc_psi(int potential, float par, float rho)
{
    const float r = rho < 0.f ? 0.f : rho;
    if (potential == LB_PSI_SHAN_CHEN) {
        const float q = r / par;
        const float ex = expf(-q);
        const float d = 1.f - ex;
        return par * d;
    }
    if (potential == LB_PSI_POW) return powf(r, par);
    return r;
}

// Stage 3, the stencil: S = sum_k w_k c_k psi(x + c_k) in the order of the links, p[row][col] with row 0 = y - 1 and col 0 = x - 1.
template <typename T>
__device__ __forceinline__ void mc_stencil_t(const T (&p)[3][3], T &sx, T &sy)
{
    const T w1 = lb_splat<T>(1.f / 9.f), w2 = lb_splat<T>(1.f / 36.f);
    const T x1 = w1 * p[1][2];
    const T x3 = lb_fma(-w1, p[1][0], x1);
    const T x5 = lb_fma(w2, p[2][2], x3);
    const T x6 = lb_fma(-w2, p[2][0], x5);
    const T x7 = lb_fma(-w2, p[0][0], x6);
    sx = lb_fma(w2, p[0][2], x7);
    const T y2 = w1 * p[2][1];
    const T y4 = lb_fma(-w1, p[0][1], y2);
    const T y5 = lb_fma(w2, p[2][2], y4);
    const T y6 = lb_fma(w2, p[2][0], y5);
    const T y7 = lb_fma(-w2, p[0][0], y6);
    sy = lb_fma(-w2, p[0][2], y7);
}

// ... and one of an entry's two increments: G += -(G_int psi) S, psi = this fluid's at the cell, S = the other fluid's stencil.
template <typename T>
__device__ __forceinline__ void mc_pair_force_t(float G_int, T psi, T sx, T sy, T &Gx, T &Gy)
{
    const T c = lb_splat<T>(G_int) * psi;
    const T nc = -c;
    Gx = lb_fma(sx, nc, Gx);
    Gy = lb_fma(sy, nc, Gy);
}

// Stage 4, one fluid's share: the running sums of update_bary_velocity's loop (link by link, then G / 2).
template <typename T>
__device__ __forceinline__ void mc_bary_add_t(const T (&f)[9], T rho, T Gx, T Gy, T &sx, T &sy, T &rs)
{
    rs = rs + rho;
    const T a1 = sx + f[1];
    const T a3 = a1 - f[3];
    const T a5 = a3 + f[5];
    const T a6 = a5 - f[6];
    const T a7 = a6 - f[7];
    const T a8 = a7 + f[8];
    sx = lb_fma(lb_splat<T>(0.5f), Gx, a8);
    const T b2 = sy + f[2];
    const T b4 = b2 - f[4];
    const T b5 = b4 + f[5];
    const T b6 = b5 + f[6];
    const T b7 = b6 - f[7];
    const T b8 = b7 - f[8];
    sy = lb_fma(lb_splat<T>(0.5f), Gy, b8);
}

// Stage 6: f_k (1 - omega) + omega feq_k + (1 - omega / 2) w_k (3 c.G + 9 (c.G)(c.u_b) - 3 u_b.G)
template <typename T>
__device__ __forceinline__ void mc_relax_t(const PmExtra &e, T (&f)[9], const T (&q)[9], float omega, T ub, T vb, T Gx, T Gy)
{
    pm_relax_t<T>(e, f, q, omega, lb_splat<T>(1.f), ub, vb, Gx, Gy);
}

// Stage 7.  add_eating_collision: phi = (a - b) / (a + b); growth = (rate a) b where |phi| < cutoff; f_eater += w growth,
// f_eatee -= w growth.
template <typename T>
__device__ __forceinline__ T mc_eat_growth_t(T ra, T rb, float rate, float cutoff)
{
    const T d = ra - rb;
    const T s = ra + rb;
    const T phi = d / s;
    const T ap = mc_abs(phi);
    const T t = lb_splat<T>(rate) * ra;
    const T g = t * rb;
    return mc_if_less(ap, lb_splat<T>(cutoff), g);
}

template <typename T>
__device__ __forceinline__ void mc_add_w_t(T (&f)[9], T g)
{
    const T w0 = lb_splat<T>(4.f / 9.f), w1 = lb_splat<T>(1.f / 9.f), w2 = lb_splat<T>(1.f / 36.f);
    f[0] = lb_fma(w0, g, f[0]);
#pragma unroll
    for (int k = 1; k < 5; ++k) f[k] = lb_fma(w1, g, f[k]);
#pragma unroll
    for (int k = 5; k < 9; ++k) f[k] = lb_fma(w2, g, f[k]);
}

// v[i] for a uniform run-time i without indexing a register array
template <typename T, int NF>
__device__ __forceinline__ T mc_pick(const T (&v)[NF], int i)
{
    T r = v[0];
#pragma unroll
    for (int n = 1; n < NF; ++n) r = i == n ? v[n] : r;
    return r;
}

// the reaction table on the populations of a cell (or a pair), in table order; rho: stage 2's
template <typename T, int NF>
__device__ __forceinline__ void mc_react_t(const McArgs &m, T (&f)[NF][9], const T (&rho)[NF])
{
    for (int t = 0; t < m.n_react; ++t) {
        const McReact r = m.react[t];
        const T ra = mc_pick<T, NF>(rho, r.a);
        T g;
        if (r.kind == LB_REACT_EAT) g = mc_eat_growth_t<T>(ra, mc_pick<T, NF>(rho, r.b), r.p0, r.p1);
        else g = mc_if_inside(ra, r.p0, r.p1, r.p2);
        const T ng = -g;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            if (n == r.a) mc_add_w_t<T>(f[n], g);
            if (r.kind == LB_REACT_EAT && n == r.b) mc_add_w_t<T>(f[n], ng);
        }
    }
}

// Stage 3 of a cell (or a pair): G_i = g_i rho_i, then the table's entries in order.  psi[t][s][row][col]: the pseudopotential of
// entry t's fluid_1 (s = 0) and fluid_2 (s = 1) around the cell.
template <typename T, int NF>
__device__ __forceinline__ void mc_entry_force_t(const McInter &t, const T (&p1)[3][3], const T (&p2)[3][3], T (&Gx)[NF], T (&Gy)[NF])
{
    T s1x, s1y, s2x, s2y;
    mc_stencil_t<T>(p1, s1x, s1y);
    mc_stencil_t<T>(p2, s2x, s2y);
#pragma unroll
    for (int n = 0; n < NF; ++n)
        if (n == t.i) mc_pair_force_t<T>(t.G, p1[1][1], s2x, s2y, Gx[n], Gy[n]);
#pragma unroll
    for (int n = 0; n < NF; ++n)
        if (n == t.j) mc_pair_force_t<T>(t.G, p2[1][1], s1x, s1y, Gx[n], Gy[n]);
}

}  // namespace
