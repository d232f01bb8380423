// nutrient.cpp -- a population and the nutrient it eats under a velocity solved from the population (the reference's
// reaction_diffusion/surfactant_nutrient_waves.py): the kernels of kernels_nutrient.h, their launches and the set calls
// lb_run_nutrient ... lb_get_nutrient_fields.  No handle kind and no row of the kind table: a set is two whole-grid periodic scalar
// lattices (LB_SEM_DIFFUSION) and an lb_spectral (spectral.cpp), the parameters travel with every call.
#include "kernels_nutrient.h"  // (first: host.h switches floating-point contraction off for what follows it, cpu_backend.h)
#include "host.h"

#include <initializer_list>

namespace {

// k_sn_step over the whole grid.  SN_ROWS = 4 rows a workgroup: the plain form is k_ad_step's launch with two lattices in a lane; the
// clumpy form stages six LDS rows for four (tools/kernel_resources.py nutrient.cpp k_sn; DESIGN.md has the table)
void sn_step(bool clumpy, bool last, hipStream_t st, const SnArgs &m)
{
    const StepArgs &a = m.a[0];
    const dim3 grid((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + SN_ROWS - 1) / SN_ROWS)), block(64, SN_ROWS);
    if (clumpy) {
        if (last) hipLaunchKernelGGL((k_sn_step<true, true>), grid, block, 0, st, m);
        else hipLaunchKernelGGL((k_sn_step<true, false>), grid, block, 0, st, m);
    } else {
        if (last) hipLaunchKernelGGL((k_sn_step<false, true>), grid, block, 0, st, m);
        else hipLaunchKernelGGL((k_sn_step<false, false>), grid, block, 0, st, m);
    }
}

// the two members of a set, checked alike for every set call
int nutrient_members(lb_sim **f, int count, const char *what)
{
    if (!f) return fail(LB_ERR_ARG, "%s: null handle array", what);
    if (count != 2) return fail(LB_ERR_ARG, "%s takes exactly 2 handles, the population and the nutrient (got a count of %d)", what, count);
    int at = 0;
    switch (set_fault(f, count, LB_SEM_DIFFUSION, true, true, &at)) {
    case SET_NULL_MEMBER: return fail(LB_ERR_ARG, "%s: null handle in the set", what);
    case SET_ROCKET_NAMED: return ROCKET_REFUSED(what);
    case SET_KIND: return fail(LB_ERR_ARG, "%s: handle %d is not a scalar lattice on the GPU (LB_SEM_DIFFUSION is required)", what, at);
    case SET_GEOMETRY: return fail(LB_ERR_ARG, "%s: the population and the nutrient must share grid (geometry), layout flag and device", what);
    case SET_SPLIT_STEP: return fail(LB_ERR_STATE, "%s inside a split step", what);
    case SET_TWICE: return fail(LB_ERR_ARG, "%s: a handle appears twice in the set", what);
    case SET_FINE: break;
    }
    for (int i = 0; i < 2; ++i) {
        if (f[i]->p.bc_mode != LB_BC_PERIODIC) return fail(LB_ERR_ARG, "%s: handle %d is not periodic (the family LB_BC_PERIODIC only)", what, i);
        if (f[i]->multi_slab()) return fail(LB_ERR_STATE, "%s is only available on handles that own the whole grid", what);
        if (f[i]->noisy) return fail(LB_ERR_STATE, "%s: handle %d has the noisy collision on (lb_set_noise), which the set's kernels do not draw", what, i);
    }
    return LB_OK;
}

int nutrient_params(lb_sim **f, const lb_nutrient_params *p, const char *what)
{
    if (!p) return fail(LB_ERR_ARG, "%s: null parameters", what);
    for (float x : {p->G, p->scale, p->rho_o, p->G_chen})
        if (!finite32(x)) return fail(LB_ERR_ARG, "%s: the parameters must be finite", what);
    if (p->clumpy) {
        if (f[0]->p.nx < 3 || f[0]->p.ny < 3) return fail(LB_ERR_ARG, "%s: the clumpy variant needs nx, ny >= 3 (every cell has eight neighbours)", what);
        if (p->rho_o == 0.f) return fail(LB_ERR_ARG, "%s: the clumpy variant needs rho_o != 0", what);
    }
    return LB_OK;
}

// psi and F of the set, with its first handle: made at first use, zero; lb_destroy frees them
int nutrient_planes(lb_sim *s)
{
    const size_t fld_bytes = sizeof(float) * s->pitch * s->H;
    for (float **q : {&s->ry_op, &s->pm_G[0], &s->pm_G[1]}) {
        if (*q) continue;
        HIP_TRY(hipMalloc(q, fld_bytes));
        HIP_TRY(hipMemsetAsync(*q, 0, fld_bytes, s->stream));
        s->bytes += fld_bytes;
    }
    return LB_OK;
}

// (src = the current lattice, dst = the other one: what the fused step reads and writes; the collision stage sets dst itself.  Every
//  derived scalar is one float32 operation, here and nowhere else: nutrient_launch.h)
SnArgs nutrient_args(lb_sim **f, const lb_nutrient_params &p)
{
    SnArgs m = {};
    for (int i = 0; i < 2; ++i) m.a[i] = step_args(f[i], 0, 1, f[i]->H);
    const float cs = (float)(1.0 / sqrt(3.0));          // np.float32(1. / np.sqrt(3))
    const float cs2 = cs * cs;
    m.inv_cs2 = (float)(1.0 / (double)cs2);             // the kernels' `1. / (cs * cs)`: a double quotient rounded once
    const float ncs2 = (-cs) * cs;                      // `-cs*cs * G_chen`, left to right
    m.kf = ncs2 * p.G_chen;
    m.G = p.G;
    m.rho_o = p.rho_o;
    m.psi = f[0]->ry_op;
    m.Fx = f[0]->pm_G[0]; m.Fy = f[0]->pm_G[1];
    return m;
}

}  // namespace

extern "C" {

int lb_run_nutrient(lb_spectral *sp, lb_sim **fields, int count, const lb_nutrient_params *p, int n_steps)
{
    int rc = nutrient_members(fields, count, "lb_run_nutrient");
    if (rc) return rc;
    lb_sim *s0 = fields[0];
    if ((rc = sp_coupled_ready(sp, s0, "lb_run_nutrient"))) return rc;
    if ((rc = nutrient_params(fields, p, "lb_run_nutrient"))) return rc;
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (n_steps == 0) return LB_OK;
    SetScope sc(fields, 2);
    if (p->clumpy && (rc = nutrient_planes(s0))) return rc;
    if ((rc = sc.join())) return rc;
    if ((rc = sp_borrow(sp, s0->stream))) return rc;
    for (int it = 0; it < n_steps; ++it) {
        if ((rc = scalar_moments(s0))) return rc;                   // rho_p after streaming; nothing moves
        if ((rc = sp_velocity_on(sp, s0, p->scale))) return rc;      // u, v of the population's handle
        sn_step(p->clumpy != 0, it == n_steps - 1, s0->stream, nutrient_args(fields, *p));
        HIP_TRY(hipGetLastError());
        for (int i = 0; i < 2; ++i) fields[i]->cur ^= 1;
    }
    set_ran(fields, 2);
    if ((rc = sp_return(sp, s0->stream))) return rc;
    return sc.release();
}

int lb_nutrient_velocity(lb_spectral *sp, lb_sim **fields, int count, float scale, int streamed)
{
    int rc = nutrient_members(fields, count, "lb_nutrient_velocity");
    if (rc) return rc;
    lb_sim *s0 = fields[0], *s1 = fields[1];
    if ((rc = sp_coupled_ready(sp, s0, "lb_nutrient_velocity"))) return rc;
    if (!finite32(scale)) return fail(LB_ERR_ARG, "the velocity's factor must be finite");
    SetScope sc(fields, 2);
    if ((rc = sc.join())) return rc;
    if (streamed) rc = scalar_moments(s0);
    else rc = ensure_macro(s0);
    if (rc) return rc;
    if ((rc = sp_borrow(sp, s0->stream))) return rc;
    if ((rc = sp_velocity_on(sp, s0, scale))) return rc;
    // (rho, u, v are [H][pitch] whatever the layout of the lattices; same pitch: same nx)
    const long long n4 = s0->pitch * s0->H / 4;
    if ((rc = copy_quads(s0->stream, s1->u, s0->u, n4))) return rc;
    if ((rc = copy_quads(s0->stream, s1->v, s0->v, n4))) return rc;
    for (int i = 0; i < 2; ++i) fields[i]->feq_valid = false;
    if ((rc = sp_return(sp, s0->stream))) return rc;
    return sc.release();
}

int lb_update_forces_nutrient(lb_sim **fields, int count, const lb_nutrient_params *p)
{
    int rc = nutrient_members(fields, count, "lb_update_forces_nutrient");
    if (rc) return rc;
    if ((rc = nutrient_params(fields, p, "lb_update_forces_nutrient"))) return rc;
    if (!p->clumpy) return fail(LB_ERR_ARG, "lb_update_forces_nutrient: psi and F exist in the clumpy variant only");
    lb_sim *s0 = fields[0];
    SetScope sc(fields, 2);
    if ((rc = nutrient_planes(s0))) return rc;
    if ((rc = sc.join())) return rc;
    const SnArgs m = nutrient_args(fields, *p);
    hipLaunchKernelGGL(k_sn_forces, cells_grid(m.a[0]), dim3(256), 0, s0->stream, m);
    HIP_TRY(hipGetLastError());
    return sc.release();
}

int lb_collide_nutrient(lb_sim **fields, int count, const lb_nutrient_params *p)
{
    int rc = nutrient_members(fields, count, "lb_collide_nutrient");
    if (rc) return rc;
    if ((rc = nutrient_params(fields, p, "lb_collide_nutrient"))) return rc;
    for (int i = 0; i < 2; ++i)
        if (!fields[i]->feq) return fail(LB_ERR_STATE, "lb_collide_nutrient before lb_update_feq on both members");
    lb_sim *s0 = fields[0];
    if (p->clumpy && !s0->ry_op) return fail(LB_ERR_STATE, "lb_collide_nutrient (clumpy) before lb_update_forces_nutrient");
    SetScope sc(fields, 2);
    if ((rc = sc.join())) return rc;
    SnArgs m = nutrient_args(fields, *p);
    for (int i = 0; i < 2; ++i) m.a[i].dst = fields[i]->origin(fields[i]->cur);      // relaxed in place
    const float *feq_p = fields[0]->feq_origin(), *feq_n = fields[1]->feq_origin();
    if (p->clumpy) hipLaunchKernelGGL(k_sn_collide<true>, cells_grid(m.a[0]), dim3(256), 0, s0->stream, m, feq_p, feq_n);
    else hipLaunchKernelGGL(k_sn_collide<false>, cells_grid(m.a[0]), dim3(256), 0, s0->stream, m, feq_p, feq_n);
    HIP_TRY(hipGetLastError());
    return sc.release();
}

int lb_get_nutrient_fields(lb_sim **fields, int count, float *psi, float *Fx, float *Fy)
{
    int rc = nutrient_members(fields, count, "lb_get_nutrient_fields");
    if (rc) return rc;
    lb_sim *s = fields[0];
    DeviceGuard guard(s->p.device);
    if ((rc = nutrient_planes(s))) return rc;       // (never made: zero, what the reference's arrays hold before update_force)
    float *out[3] = {psi, Fx, Fy};
    const float *from[3] = {s->ry_op, s->pm_G[0], s->pm_G[1]};
    for (int i = 0; i < 3; ++i)
        if (out[i] && (rc = copy_plane_d2h(s, out[i], from[i]))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

}  // extern "C"
