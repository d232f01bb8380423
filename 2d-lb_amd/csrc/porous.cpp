// porous.cpp -- forced flow in a porous medium (LB_SEM_POROUS): the kernels of kernels_porous.h and their launches, the kind's row of the
// kind table (host.h: KindOps), its run, and the entry points of the C ABI that are its own or that a fluid of a multicomponent set
// shares with it: lb_set_porous, the body force, the force field, G and u_b.
#include "kernels_porous.h"    // (first: host.h switches floating-point contraction off for what follows it, cpu_backend.h)
#include "host.h"

#include <initializer_list>

namespace {

// the fused step over the whole grid; last: this launch stores rho, u, v, G and u_b
template <int BC>
void pm_step(bool field, bool last, hipStream_t st, const StepArgs &a, const PmExtra &e)
{
    const dim3 block(64, 4), grid = step_grid(a);
    if (field) {
        if (last) hipLaunchKernelGGL((k_pm_step<BC, true, true>), grid, block, 0, st, a, e);
        else hipLaunchKernelGGL((k_pm_step<BC, true, false>), grid, block, 0, st, a, e);
    } else {
        if (last) hipLaunchKernelGGL((k_pm_step<BC, false, true>), grid, block, 0, st, a, e);
        else hipLaunchKernelGGL((k_pm_step<BC, false, false>), grid, block, 0, st, a, e);
    }
}

int porous_hydro(lb_sim *s) { return launch_phase(s, grid_cells(s), k_pm_hydro); }       // rho, and u, v where rho > 1e-6

// f relaxed in place towards feq, plus the forcing
int porous_collide(lb_sim *s)
{
    int rc = collide_ready(s);
    return rc ? rc : launch_phase(s, grid_cells(s), k_pm_collide, pm_extra(s), s->origin(s->cur), s->feq_origin());
}

// n time steps: k_pm_step, one launch each; the last stores rho, u, v, the total force and the barycentric velocity
int run_porous(lb_sim *s, int n_steps)
{
    const PmExtra e = pm_extra(s);
    for (int it = 0; it < n_steps; ++it) {
        const StepArgs a = step_args(s, 0, 1, s->H);
        if (s->p.bc_mode == LB_BC_PERIODIC) pm_step<LB_BC_PERIODIC>(e.fgx != nullptr, it == n_steps - 1, s->stream, a, e);
        else pm_step<LB_BC_ZERO_GRADIENT>(e.fgx != nullptr, it == n_steps - 1, s->stream, a, e);
        HIP_TRY(hipGetLastError());
        s->cur ^= 1;
    }
    if (n_steps) { s->feq_valid = false; s->macro_valid = true; }
    return LB_OK;
}

int pm_get_pair(lb_sim *s, float *const (&pair)[2], float *a, float *b)
{
    DeviceGuard guard(s->p.device);
    int rc;
    if (a && (rc = copy_plane_d2h(s, a, pair[0]))) return rc;
    if (b && (rc = copy_plane_d2h(s, b, pair[1]))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int pm_set_pair(lb_sim *s, float *const (&pair)[2], const float *a, const float *b)
{
    if (!a || !b) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    int rc;
    if ((rc = copy_plane_h2d(s, pair[0], a))) return rc;
    if ((rc = copy_plane_h2d(s, pair[1], b))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

}  // namespace

// (every derived scalar one float32 operation, here and nowhere else: porous_launch.h)
PmExtra pm_extra(const lb_sim *s)
{
    PmExtra e;
    e.Gx = s->pm_G[0]; e.Gy = s->pm_G[1];
    e.ub = s->pm_ub[0]; e.vb = s->pm_ub[1];
    e.fgx = s->pm_field[0]; e.fgy = s->pm_field[1];
    e.gx = s->pm_gx; e.gy = s->pm_gy;
    e.eps = s->pm_eps;
    e.en = s->pm_eps * s->pm_nu;
    e.ef = s->pm_eps * s->pm_Fe;
    e.K = s->pm_K;
    e.sqrtK = sqrtf(s->pm_K);
    const float ie = 1.f / s->pm_eps;
    e.a15 = 1.5f * ie; e.a45 = 4.5f * ie;
    e.b3 = 3.f * ie; e.b9 = 9.f * ie;
    e.hw = 1.f - 0.5f * s->p.omega;
    return e;
}

int forced_create(lb_sim *s)
{
    s->diag = 0;                                // (the diagnostic word of the flow kernels means nothing here)
    const size_t fld_bytes = sizeof(float) * s->pitch * s->H;
    for (float **q : {&s->pm_G[0], &s->pm_G[1], &s->pm_ub[0], &s->pm_ub[1]}) {
        CREATE_TRY(hipMalloc(q, fld_bytes));
        CREATE_TRY(hipMemsetAsync(*q, 0, fld_bytes, s->stream));
    }
    s->bytes += 4 * fld_bytes;
    return LB_OK;
}

// single_component.cl's and multi.cl's move_open_bcs: boundary cells copy their interior neighbour, in place (single_component.py:155-156:
// `pass` in the periodic family)
int porous_move_bcs(lb_sim *s) { return s->p.bc_mode == LB_BC_PERIODIC ? LB_OK : launch_phase(s, grid_edge(s), k_pm_move_bcs, s->origin(s->cur)); }
// from rho and u_b (a fluid of a multicomponent set: epsilon = 1)
int porous_feq(lb_sim *s) { return launch_phase(s, grid_cells(s), k_pm_feq, pm_extra(s), s->feq_origin()); }

KIND_ROW(kind_porous,
    "forced flow in a porous medium (LB_SEM_POROUS)", 1u << LB_BC_PERIODIC | 1u << LB_BC_ZERO_GRADIENT, "the families LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT only", false, true,
    0, "lb_set_variant: a porous-medium fluid (LB_SEM_POROUS) takes the variants -1 and 0 only: k_pm_step, no tiles", LB_ERR_STATE,
    forced_create, porous_move_bcs, porous_hydro, porous_feq, porous_collide, run_porous)

#define NEED_POROUS(s, name)                                                                                 \
    do {                                                                                                     \
        if (!(s)) return fail(LB_ERR_ARG, "null handle");                                                    \
        NOT_ROCKET(s, name);                                                                                 \
        if ((s)->multifluid()) return fail(LB_ERR_STATE, "%s is not available on a fluid of a multicomponent set (LB_SEM_MULTIFLUID)", name); \
        if (!(s)->porous()) return fail(LB_ERR_STATE, "%s is for forced flow in a porous medium (LB_SEM_POROUS)", name); \
    } while (0)
// (the calls a fluid of a multicomponent set shares with the porous-medium fluid: its g, its force field, G and u_b)
#define NEED_FORCED(s, name)                                                                                 \
    do {                                                                                                     \
        if (!(s)) return fail(LB_ERR_ARG, "null handle");                                                    \
        NOT_ROCKET(s, name);                                                                                 \
        if (!(s)->porous() && !(s)->multifluid())                                                            \
            return fail(LB_ERR_STATE, "%s is for forced flow in a porous medium (LB_SEM_POROUS) and the fluids of a multicomponent set (LB_SEM_MULTIFLUID)", name); \
    } while (0)

extern "C" {

int lb_set_porous(lb_sim *s, float epsilon, float nu_fluid, float K, float Fe)
{
    NEED_POROUS(s, "lb_set_porous");
    if (!finite32(epsilon) || !finite32(nu_fluid) || !finite32(K) || !finite32(Fe)) return fail(LB_ERR_ARG, "epsilon, nu_fluid, K and Fe must be finite");
    if (!(epsilon > 0.f) || !(K > 0.f)) return fail(LB_ERR_ARG, "need epsilon > 0 and K > 0 (got %g, %g)", epsilon, K);
    s->pm_eps = epsilon; s->pm_nu = nu_fluid; s->pm_K = K; s->pm_Fe = Fe;
    s->feq_valid = false;
    return LB_OK;
}

int lb_set_body_force(lb_sim *s, float gx, float gy)
{
    NEED_FORCED(s, "lb_set_body_force");
    if (!finite32(gx) || !finite32(gy)) return fail(LB_ERR_ARG, "the body force must be finite");
    s->pm_gx = gx; s->pm_gy = gy;
    return LB_OK;
}

int lb_set_force_field(lb_sim *s, const float *gx, const float *gy, int on_device)
{
    NEED_FORCED(s, "lb_set_force_field");
    if ((gx == nullptr) != (gy == nullptr)) return fail(LB_ERR_ARG, "both planes of the force field, or neither");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipStreamSynchronize(s->stream));       // (kernels of an un-waited run may still be reading it)
    if (!gx) {
        for (float *&q : s->pm_field) {
            if (q) {
                HIP_TRY(hipFree(q));
                s->bytes -= (int64_t)sizeof(float) * s->pitch * s->H;
            }
            q = nullptr;
        }
        s->has_field = false;
        return LB_OK;
    }
    const size_t fld_bytes = sizeof(float) * s->pitch * s->H;
    const float *from[2] = {gx, gy};
    for (int i = 0; i < 2; ++i) {
        if (!s->pm_field[i]) {
            HIP_TRY(hipMalloc(&s->pm_field[i], fld_bytes));
            s->bytes += (int64_t)fld_bytes;
        }
        HIP_TRY(hipMemsetAsync(s->pm_field[i], 0, fld_bytes, s->stream));
        HIP_TRY(hipMemcpy2DAsync(s->pm_field[i], s->pitch * sizeof(float), from[i], s->p.nx * sizeof(float), s->p.nx * sizeof(float), s->H,
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->has_field = true;
    return LB_OK;
}

int lb_get_force(lb_sim *s, float *Gx, float *Gy)
{
    NEED_FORCED(s, "lb_get_force");
    return pm_get_pair(s, s->pm_G, Gx, Gy);
}

int lb_get_bary_velocity(lb_sim *s, float *u_bary, float *v_bary)
{
    NEED_FORCED(s, "lb_get_bary_velocity");
    return pm_get_pair(s, s->pm_ub, u_bary, v_bary);
}

int lb_set_bary_velocity(lb_sim *s, const float *u_bary, const float *v_bary)
{
    NEED_FORCED(s, "lb_set_bary_velocity");
    int rc = pm_set_pair(s, s->pm_ub, u_bary, v_bary);
    if (!rc) s->feq_valid = false;
    return rc;
}

// (checkpoints: the total force as the last step left it)
int lb_set_force(lb_sim *s, const float *Gx, const float *Gy)
{
    NEED_FORCED(s, "lb_set_force");
    return pm_set_pair(s, s->pm_G, Gx, Gy);
}

int lb_update_forces(lb_sim *s)                     // G from rho, u, v
{
    NEED_FORCED(s, "lb_update_forces");
    if (s->multifluid()) return lb_update_forces_fluids(&s, 1);
    DeviceGuard guard(s->p.device);
    return launch_phase(s, grid_cells(s), k_pm_forces, pm_extra(s));
}

int lb_update_bary_velocity(lb_sim *s)              // u_b from the current lattice, rho and G
{
    NEED_FORCED(s, "lb_update_bary_velocity");
    if (s->multifluid()) return lb_update_bary_fluids(&s, 1);
    DeviceGuard guard(s->p.device);
    int rc = launch_phase(s, grid_cells(s), k_pm_bary, pm_extra(s), s->origin(s->cur));
    if (!rc) s->feq_valid = false;
    return rc;
}

}  // extern "C"
