// scalar_cell.h -- device-side arithmetic of one cell of a SCALAR lattice (LB_SEM_DIFFUSION): the reference's
// LB_D2Q9/D2Q9_diffusion.cl -- update_hydro_diffusion :41-68 (rho = sum f; u, v imposed), update_feq_diffusion :1-38 (the linear
// equilibrium feq_k = w_k rho (1 + c_k.u / cs^2)), collide_particles :70-93 and collide_particles_fisher :95-124 (+ w_k G rho (1 - rho)).
// Written once for a scalar cell (T = float) and for a pair of x-adjacent cells (T = f2a), in the style of d2q9_cell.h: the same
// operations in the same order with explicit fma, so a cell gets the same bits whichever form, and whichever kernel, computes it.
//
// 1 / cs^2: the reference divides c_k.u by cs*cs of the float32 cs = fl(1 / sqrt(3)); here it is the constant 3, once (ad_relax_t and
// ad_feq_t below): no division in the cell.  A numpy model with the constant 3 followed the reference's C to 1.0e-7 after 1000 steps.
#pragma once
#include "d2q9_cell.h"
#include "philox.h"

namespace {

template <typename T>
__device__ __forceinline__ T ad_rho_t(T f0, T f1, T f2, T f3, T f4, T f5, T f6, T f7, T f8)
{
    return f0 + f1 + f2 + f3 + f4 + f5 + f6 + f7 + f8;        // D2Q9_diffusion.cl:66, left to right
}

// omega feq_k for the pair of links +-c: r (1 +- 3 cu) as fma(+-3r, cu, r), r = fl(w) (omega rho)
template <typename T>
__device__ __forceinline__ void ad_feq_pair(T r, T r3, T cu, T &fp, T &fm)
{
    fp = lb_fma(r3, cu, r);
    fm = lb_fma(-r3, cu, r);
}

// The growth term of one cell / one pair, added last: fl(w_k) ((G rho) room), room = 1 - rho for a lattice on its own
// (D2Q9_diffusion.cl:112, 121), 1 - (rho_0 + rho_1 + ...) for a field of a coupled set (D2Q9_multifield_fisher.cl:
// collide_particles).  With one field the two are the same bits.
template <typename T>
__device__ __forceinline__ void ad_grow_t(T &f0, T &f1, T &f2, T &f3, T &f4, T &f5, T &f6, T &f7, T &f8, float G, T rho, T room)
{
    const T react = (lb_splat<T>(G) * rho) * room;
    const T w0 = lb_splat<T>(4.f / 9.f), w1 = lb_splat<T>(1.f / 9.f), w2 = lb_splat<T>(1.f / 36.f);
    f0 = lb_fma(w0, react, f0);
    f1 = lb_fma(w1, react, f1);
    f3 = lb_fma(w1, react, f3);
    f2 = lb_fma(w1, react, f2);
    f4 = lb_fma(w1, react, f4);
    f5 = lb_fma(w2, react, f5);
    f7 = lb_fma(w2, react, f7);
    f8 = lb_fma(w2, react, f8);
    f6 = lb_fma(w2, react, f6);
}

// Equilibrium and relaxation (and, REACT, the growth term) of one cell / one pair, in place.  omega enters once, through the
// density, as in equilibrate_t: every equilibrium below comes out as omega feq_k, the float32 weights multiply a run-time value.
template <typename T, bool REACT>
__device__ __forceinline__ void ad_relax_t(T &f0, T &f1, T &f2, T &f3, T &f4, T &f5, T &f6, T &f7, T &f8, float omega, float G,
                                           T rho, T ux, T uy)
{
    const T keep = lb_splat<T>(1.f - omega);
    const T rw = lb_splat<T>(omega) * rho;
    const T r0 = (4.f / 9.f) * rw, r1 = (1.f / 9.f) * rw, r2 = (1.f / 36.f) * rw;
    const T r13 = 3.f * r1, r23 = 3.f * r2;
    T e1, e2, e3, e4, e5, e6, e7, e8;
    ad_feq_pair<T>(r1, r13, ux, e1, e3);
    ad_feq_pair<T>(r1, r13, uy, e2, e4);
    ad_feq_pair<T>(r2, r23, ux + uy, e5, e7);
    ad_feq_pair<T>(r2, r23, ux - uy, e8, e6);
    f0 = lb_fma(f0, keep, r0);
    f1 = lb_fma(f1, keep, e1);
    f3 = lb_fma(f3, keep, e3);
    f2 = lb_fma(f2, keep, e2);
    f4 = lb_fma(f4, keep, e4);
    f5 = lb_fma(f5, keep, e5);
    f7 = lb_fma(f7, keep, e7);
    f8 = lb_fma(f8, keep, e8);
    f6 = lb_fma(f6, keep, e6);
    if (REACT) ad_grow_t<T>(f0, f1, f2, f3, f4, f5, f6, f7, f8, G, rho, lb_splat<T>(1.f) - rho);
}

// ---- the noisy collision: collide_particles_noisy_fisher, D2Q9_diffusion.cl:127-167 --------------------------------------------------
// Two normals from two words of the stream (philox.h): R cos(theta), R sin(theta), R = sqrt(-2 ln u(ra)), theta = 2 pi u(rb).  The one
// place where the logarithm, the square root and the sine / cosine are written: every kernel inlines it, so a cell's normal is the same
// bits wherever it is (re)computed.  Library routines throughout (the argument of sincospif, 2 u, is exact): held to a float64 model by
// tests/test_gpu_noise.py.
__device__ __forceinline__ void ad_normal_pair(uint32_t ra, uint32_t rb, float &zc, float &zs)
{
    const float radius = sqrtf(-2.f * logf(philox_uniform(ra)));
    float sn, cs;
    sincospif(2.f * philox_uniform(rb), &sn, &cs);
    zc = radius * cs;
    zs = radius * sn;
}

// the normals of the lane-of-four at box cells x4 .. x4+3 of row y
__device__ __forceinline__ void ad_lane_normals(unsigned long long seed, int x4, int y, unsigned long long t, float (&z)[4])
{
    uint32_t r[4];
    philox_lane_words(seed, x4, y, t, r);
    ad_normal_pair(r[0], r[1], z[0], z[1]);
    ad_normal_pair(r[2], r[3], z[2], z[3]);
}

// ... of the one box cell (x, y): its lane's words, its pair, its half of the pair
__device__ __forceinline__ float ad_cell_normal(unsigned long long seed, int x, int y, unsigned long long t)
{
    uint32_t r[4];
    philox_lane_words(seed, x, y, t, r);
    const bool second = (x & 2) != 0;
    float zc, zs;
    ad_normal_pair(second ? r[2] : r[0], second ? r[3] : r[1], zc, zs);
    return (x & 1) ? zs : zc;
}

__device__ __forceinline__ float ad_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ f2a ad_sqrt(f2a x) { return f2a{sqrtf(x.x), sqrtf(x.y)}; }
// new_f < 0 -> 0 as a compare-and-select: false for NaN, which stays (the reference's `if (new_f < 0) new_f = 0`; not fmaxf)
__device__ __forceinline__ float ad_clamp0(float x) { return x < 0.f ? 0.f : x; }
__device__ __forceinline__ f2a ad_clamp0(f2a x) { return f2a{x.x < 0.f ? 0.f : x.x, x.y < 0.f ? 0.f : x.y}; }

// react = G rho (1 - rho) + sqrt(Dg rho (1 - rho)) z, each product and the sum rounded on its own as the reference's C does; rho
// outside [0, 1] makes the root, react and all nine links NaN, as there
template <typename T>
__device__ __forceinline__ T ad_noisy_react_t(float G, float Dg, T rho, T z)
{
    const T room = lb_splat<T>(1.f) - rho;
    const T grow = (lb_splat<T>(G) * rho) * room;
    const T root = ad_sqrt((lb_splat<T>(Dg) * rho) * room);
    const T kick = root * z;
    return grow + kick;
}

// The noisy form of ad_relax_t: the plain relaxation, then fl(w_k) react added last as the growth term is (ad_grow_t's order), then
// the clamp.
template <typename T>
__device__ __forceinline__ void ad_relax_noisy_t(T &f0, T &f1, T &f2, T &f3, T &f4, T &f5, T &f6, T &f7, T &f8, float omega, float G,
                                                 float Dg, T rho, T ux, T uy, T z)
{
    ad_relax_t<T, false>(f0, f1, f2, f3, f4, f5, f6, f7, f8, omega, G, rho, ux, uy);
    const T react = ad_noisy_react_t<T>(G, Dg, rho, z);
    const T w0 = lb_splat<T>(4.f / 9.f), w1 = lb_splat<T>(1.f / 9.f), w2 = lb_splat<T>(1.f / 36.f);
    f0 = ad_clamp0(lb_fma(w0, react, f0));
    f1 = ad_clamp0(lb_fma(w1, react, f1));
    f3 = ad_clamp0(lb_fma(w1, react, f3));
    f2 = ad_clamp0(lb_fma(w1, react, f2));
    f4 = ad_clamp0(lb_fma(w1, react, f4));
    f5 = ad_clamp0(lb_fma(w2, react, f5));
    f7 = ad_clamp0(lb_fma(w2, react, f7));
    f8 = ad_clamp0(lb_fma(w2, react, f8));
    f6 = ad_clamp0(lb_fma(w2, react, f6));
}

// ---- strains on a shared nutrient: D2Q9_multifield_diffusion.cl (kernels_expansion.h) -------------------------------------------------
// update_hydro's cutoff: rho < cut or NaN -> 0, as compares and selects (the NaN test is explicit)
__device__ __forceinline__ float ex_cut(float rho, float cut) { return (rho < cut || rho != rho) ? 0.f : rho; }
__device__ __forceinline__ f2a ex_cut(f2a rho, float cut) { return f2a{ex_cut(rho.x, cut), ex_cut(rho.y, cut)}; }
// collide_particles' floor: the link becomes 0 where its field's (cut) rho < cut, where the new value < 0 or where it is NaN
__device__ __forceinline__ float ex_floor(float v, float rho, float cut) { return (rho < cut || v < 0.f || v != v) ? 0.f : v; }
__device__ __forceinline__ f2a ex_floor(f2a v, f2a rho, float cut) { return f2a{ex_floor(v.x, rho.x, cut), ex_floor(v.y, rho.y, cut)}; }

// react of one strain on the nutrient c: growth = (G rho) c; NOISY: + sqrt((Dg rho) c) z + ((Dg c) / 4) (z z - 1), the Milstein term.
// Each product and each sum is a float32 of its own (one operation a statement: nothing contracts); the reference's `4.` and `1.`
// make its Milstein term a double product -- the float32 one here is inside the contract's tolerance.
template <typename T, bool NOISY>
__device__ __forceinline__ T ex_react_t(float G, float Dg, T rho, T c, T z)
{
    const T gr = lb_splat<T>(G) * rho;
    const T growth = gr * c;
    if (!NOISY) return growth;
    const T dr = lb_splat<T>(Dg) * rho;
    const T drc = dr * c;
    const T kick = ad_sqrt(drc) * z;
    const T dc = lb_splat<T>(Dg) * c;
    const T quarter = dc * lb_splat<T>(0.25f);
    const T zz = z * z;
    const T zz1 = zz - lb_splat<T>(1.f);
    const T mil = quarter * zz1;
    const T fluct = kick + mil;
    return growth + fluct;
}

// the relaxation of one member towards the equilibrium of its cut rho (ad_relax_t: omega enters through rho), fl(w_k) react added last
// in ad_grow_t's order, then the floor
template <typename T>
__device__ __forceinline__ void ex_relax_t(T &f0, T &f1, T &f2, T &f3, T &f4, T &f5, T &f6, T &f7, T &f8, float omega, float cut, T rho,
                                           T ux, T uy, T react)
{
    ad_relax_t<T, false>(f0, f1, f2, f3, f4, f5, f6, f7, f8, omega, 0.f, rho, ux, uy);
    const T w0 = lb_splat<T>(4.f / 9.f), w1 = lb_splat<T>(1.f / 9.f), w2 = lb_splat<T>(1.f / 36.f);
    f0 = ex_floor(lb_fma(w0, react, f0), rho, cut);
    f1 = ex_floor(lb_fma(w1, react, f1), rho, cut);
    f3 = ex_floor(lb_fma(w1, react, f3), rho, cut);
    f2 = ex_floor(lb_fma(w1, react, f2), rho, cut);
    f4 = ex_floor(lb_fma(w1, react, f4), rho, cut);
    f5 = ex_floor(lb_fma(w2, react, f5), rho, cut);
    f7 = ex_floor(lb_fma(w2, react, f7), rho, cut);
    f8 = ex_floor(lb_fma(w2, react, f8), rho, cut);
    f6 = ex_floor(lb_fma(w2, react, f6), rho, cut);
}

// feq_k itself (the un-fused update_feq_diffusion): ad_relax_t's equilibrium with omega = 1
__device__ __forceinline__ void ad_feq_cell(float (&e)[9], float rho, float ux, float uy)
{
    const float r0 = (4.f / 9.f) * rho, r1 = (1.f / 9.f) * rho, r2 = (1.f / 36.f) * rho;
    const float r13 = 3.f * r1, r23 = 3.f * r2;
    e[0] = r0;
    ad_feq_pair<float>(r1, r13, ux, e[1], e[3]);
    ad_feq_pair<float>(r1, r13, uy, e[2], e[4]);
    ad_feq_pair<float>(r2, r23, ux + uy, e[5], e[7]);
    ad_feq_pair<float>(r2, r23, ux - uy, e[8], e[6]);
}

// ---- the Poisson relaxation (LB_SEM_POISSON): the reference's LB_D2Q9/D2Q9_poisson.cl -- update_hydro :34-63 (rho = (9/5)(f1 + ... + f8);
// f0 is not read), update_feq :1-31 (feq_0 = (w0 - 1) rho, feq_k = w_k rho), collide_particles :65-97 (f_k (1 - omega) + omega feq_k +
// w_k react).  Unlike the transport cell above, the fused step and the un-fused phases are held to each other BITWISE: both go through
// these three functions, feq_k is a float32 of its own (stored by the phases, a register of the fused cell), and omega multiplies it.
template <typename T>
__device__ __forceinline__ T ps_rho_t(T f1, T f2, T f3, T f4, T f5, T f6, T f7, T f8)
{
    return (9.f / 5.f) * (f1 + f2 + f3 + f4 + f5 + f6 + f7 + f8);     // D2Q9_poisson.cl:59, left to right
}

template <typename T>
__device__ __forceinline__ void ps_feq_t(T (&e)[9], T rho)
{
    const float w0 = 4.f / 9.f, w1 = 1.f / 9.f, w2 = 1.f / 36.f;
    e[0] = (w0 - 1.f) * rho;
    e[1] = w1 * rho; e[2] = w1 * rho; e[3] = w1 * rho; e[4] = w1 * rho;
    e[5] = w2 * rho; e[6] = w2 * rho; e[7] = w2 * rho; e[8] = w2 * rho;
}

// f_k := fma(w_k, react, fma(f_k, 1 - omega, omega feq_k)), in place; react = source x (delta_t D), one float32 per cell
template <typename T>
__device__ __forceinline__ void ps_relax_t(T (&f)[9], const T (&e)[9], float omega, T react)
{
    const T keep = lb_splat<T>(1.f - omega), om = lb_splat<T>(omega);
    const T w[9] = {lb_splat<T>(4.f / 9.f), lb_splat<T>(1.f / 9.f), lb_splat<T>(1.f / 9.f), lb_splat<T>(1.f / 9.f), lb_splat<T>(1.f / 9.f),
                    lb_splat<T>(1.f / 36.f), lb_splat<T>(1.f / 36.f), lb_splat<T>(1.f / 36.f), lb_splat<T>(1.f / 36.f)};
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = lb_fma(w[k], react, lb_fma(f[k], keep, om * e[k]));
}

}  // namespace
