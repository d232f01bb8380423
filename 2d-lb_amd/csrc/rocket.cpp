// rocket.cpp -- surfactant-propelled colonies (LB_SEM_ROCKET): the kernels of kernels_rocket.h and their launches, the kind's row of the
// kind table (host.h: KindOps) and the set calls lb_set_rocket ... lb_get_rocket_fields.
#include "kernels_rocket.h"    // (first: host.h switches floating-point contraction off for what follows it, cpu_backend.h)
#include "host.h"

#include <initializer_list>

namespace {

template <int MODE>
void launch_collide(bool last, hipStream_t st, const RyArgs &m)
{
    if (last) hipLaunchKernelGGL((k_ry_collide<MODE, true>), step_grid(m.a[0]), dim3(64, 4), 0, st, m);
    else hipLaunchKernelGGL((k_ry_collide<MODE, false>), step_grid(m.a[0]), dim3(64, 4), 0, st, m);
}

// RY_ROWS (plan_consts.h) = 10 rows a workgroup: the cell of two lattices with both operands around it takes 134-162 registers, which
// leaves three waves a SIMD, twelve a CU -- one workgroup of 10 + 2 waves fills it and gathers 12 rows for 10
// (tools/kernel_resources.py rocket.cpp k_ry; DESIGN.md section 14 has the table and what 6 and 4 rows measured)
template <int MODE>
void launch_fused(bool last, hipStream_t st, const RyArgs &m)
{
    constexpr int R = RY_ROWS;
    const StepArgs &a = m.a[0];
    const dim3 grid((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + R - 1) / R)), block(64, R + 2);
    if (last) hipLaunchKernelGGL((k_ry_step<MODE, R, true>), grid, block, 0, st, m);
    else hipLaunchKernelGGL((k_ry_step<MODE, R, false>), grid, block, 0, st, m);
}

// mode = LB_ROCKET_FLOW or LB_ROCKET_FORCES.
// The two-launch step: k_ry_moments stores both densities, k_ry_collide gathers again, reads the densities around the cell and runs
// stages 3-5; last: it also stores u, v, psi / S and the forces.
void ry_collide(int mode, bool last, hipStream_t st, const RyArgs &m)
{
    if (mode == LB_ROCKET_FLOW) launch_collide<LB_ROCKET_FLOW>(last, st, m);
    else launch_collide<LB_ROCKET_FORCES>(last, st, m);
}

// The one-launch step k_ry_step: a workgroup owns RY_ROWS rows of a 256-cell tile and keeps the two stencil operands of them, of one
// halo row above and below and of one halo cell left and right in LDS; last: it also stores rho, u, v, psi / S and the forces.
// Bitwise the two-launch step.
void ry_step(int mode, bool last, hipStream_t st, const RyArgs &m)
{
    if (mode == LB_ROCKET_FLOW) launch_fused<LB_ROCKET_FLOW>(last, st, m);
    else launch_fused<LB_ROCKET_FORCES>(last, st, m);
}

int rocket_create(lb_sim *s)
{
    int rc = forced_create(s);                      // pm_G: the pseudo-force / the pressure force; pm_ub: the surface force
    if (rc) return rc;
    // (every handle can be a set's first: psi / S and the forces of the last step live there)
    const size_t fld_bytes = sizeof(float) * s->pitch * s->H;
    CREATE_TRY(hipMalloc(&s->ry_op, fld_bytes));
    CREATE_TRY(hipMemsetAsync(s->ry_op, 0, fld_bytes, s->stream));
    s->bytes += fld_bytes;
    return LB_OK;
}

int rocket_collide(lb_sim *s) { NOT_ROCKET(s, "lb_collide_particles (the collision needs both members: lb_collide_rocket)"); return LB_OK; }
int rocket_run(lb_sim *s, int) { NOT_ROCKET(s, "lb_run (a colony advances as a set of two: lb_run_rocket)"); return LB_OK; }

// the two members of a set, checked alike for every set call
int rocket_members(lb_sim **f, int count, const char *what)
{
    if (!f) return fail(LB_ERR_ARG, "%s: null handle array", what);
    if (count != 2) return fail(LB_ERR_ARG, "%s takes exactly 2 handles, the population and the surfactant (got a count of %d)", what, count);
    int at = 0;
    switch (set_fault(f, count, LB_SEM_ROCKET, false, true, &at)) {
    case SET_NULL_MEMBER: return fail(LB_ERR_ARG, "%s: null handle in the set", what);
    case SET_KIND: return fail(LB_ERR_ARG, "%s: handle %d is not a lattice of a surfactant-propelled colony (a non-rocket handle: LB_SEM_ROCKET is required)", what, at);
    case SET_GEOMETRY: return fail(LB_ERR_ARG, "%s: the two lattices of a colony must share grid (geometry), layout flag and device", what);
    case SET_SPLIT_STEP: return fail(LB_ERR_STATE, "%s inside a split step", what);
    case SET_TWICE: return fail(LB_ERR_ARG, "%s: a handle appears twice in the set", what);
    default: return LB_OK;
    }
}

// (src = the current lattice, dst = the other one: what the fused steps read and write; the stages set dst themselves.  Every derived
//  scalar is one float32 operation, here and nowhere else: rocket_launch.h)
RyArgs rocket_args(lb_sim **f)
{
    RyArgs m = {};
    for (int i = 0; i < 2; ++i) m.a[i] = step_args(f[i], 0, 1, f[i]->H);
    const lb_rocket_params &r = f[0]->ry;
    const float cs = (float)(1.0 / sqrt(3.0));          // np.float32(1. / np.sqrt(3))
    const float cs2 = cs * cs;
    m.inv_cs2 = (float)(1.0 / (double)cs2);             // the kernels' `1. / (cs * cs)`: a double quotient rounded once
    m.G = r.G; m.Gc = r.G_c;
    m.ke = (-r.epsilon) * m.inv_cs2;
    m.ngc = -r.G_chen;
    m.rho_o = r.rho_o; m.c_o = r.c_o; m.alpha = r.alpha;
    m.op = f[0]->ry_op;
    m.Fx = f[0]->pm_G[0]; m.Fy = f[0]->pm_G[1];
    m.Sx = f[0]->pm_ub[0]; m.Sy = f[0]->pm_ub[1];
    return m;
}

}  // namespace

// (move_bcs: the periodic family has none; hydro and feq are a scalar lattice's; the collision and a run need both members)
KIND_ROW(kind_rocket,
    "a lattice of a surfactant-propelled colony (LB_SEM_ROCKET)", 1u << LB_BC_PERIODIC, "the family LB_BC_PERIODIC only (box boundaries are not built)", true, true,
    1, "lb_set_variant: a lattice of a surfactant-propelled colony (LB_SEM_ROCKET) takes the variants -1 (the planner's choice), 0 (the two-launch step k_ry_moments + k_ry_collide) and 1 (the one-launch step k_ry_step) only", LB_ERR_STATE,
    rocket_create, nullptr, scalar_hydro, scalar_feq, rocket_collide, rocket_run)

extern "C" {

int lb_set_rocket(lb_sim **fields, int count, const lb_rocket_params *params)
{
    int rc = rocket_members(fields, count, "lb_set_rocket");
    if (rc) return rc;
    if (!params) return fail(LB_ERR_ARG, "lb_set_rocket: null parameters");
    const lb_rocket_params &r = *params;
    if (r.mode != LB_ROCKET_FLOW && r.mode != LB_ROCKET_FORCES) return fail(LB_ERR_ARG, "lb_set_rocket: unknown mode %d (LB_ROCKET_FLOW and LB_ROCKET_FORCES are built)", r.mode);
    for (float x : {r.G, r.G_c, r.epsilon, r.rho_o, r.G_chen, r.c_o, r.alpha})
        if (!finite32(x)) return fail(LB_ERR_ARG, "lb_set_rocket: the parameters must be finite");
    if (r.mode == LB_ROCKET_FLOW && r.rho_o == 0.f) return fail(LB_ERR_ARG, "lb_set_rocket: LB_ROCKET_FLOW needs rho_o != 0");
    if (r.mode == LB_ROCKET_FORCES && r.c_o == 0.f) return fail(LB_ERR_ARG, "lb_set_rocket: LB_ROCKET_FORCES needs c_o != 0");
    fields[0]->ry = r;
    return LB_OK;
}

int lb_get_rocket(lb_sim *first, lb_rocket_params *params)
{
    if (!first || !params) return fail(LB_ERR_ARG, "null argument");
    if (first->cpu || !first->rocket()) return fail(LB_ERR_STATE, "lb_get_rocket is for the lattices of a surfactant-propelled colony (LB_SEM_ROCKET)");
    *params = first->ry;
    return LB_OK;
}

int lb_run_rocket(lb_sim **fields, int count, int n_steps)
{
    int rc = rocket_members(fields, count, "lb_run_rocket");
    if (rc) return rc;
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (n_steps == 0) return LB_OK;
    lb_sim *s0 = fields[0];
    SetScope sc(fields, 2);
    if ((rc = sc.join())) return rc;
    const int mode = s0->ry.mode;
    for (int it = 0; it < n_steps; ++it) {
        const RyArgs m = rocket_args(fields);
        const bool last = it == n_steps - 1;            // the last launch stores rho, u, v, psi / S and the forces
        if (rocket_one_launch(s0)) {                    // (the set's first handle chooses: lb_set_variant; plan.cpp)
            ry_step(mode, last, s0->stream, m);
            HIP_TRY(hipGetLastError());
        } else {
            hipLaunchKernelGGL(k_ry_moments, step_grid(m.a[0]), dim3(64, 4), 0, s0->stream, m);
            HIP_TRY(hipGetLastError());
            ry_collide(mode, last, s0->stream, m);
            HIP_TRY(hipGetLastError());
        }
        for (int i = 0; i < 2; ++i) fields[i]->cur ^= 1;
    }
    set_ran(fields, 2);
    return sc.release();
}

// The un-fused stage 3 and stage 5, from the stored densities: u, v (FLOW: the stencil over rho_c; FORCES: F_p + F_s from the stored
// forces); psi / S and the forces; both lattices relaxed in place towards their feq
int lb_update_velocity_rocket(lb_sim **fields, int count)
{
    int rc = rocket_members(fields, count, "lb_update_velocity_rocket");
    if (rc) return rc;
    SetScope sc(fields, 2);
    if ((rc = sc.join())) return rc;
    const RyArgs m = rocket_args(fields);
    if (fields[0]->ry.mode == LB_ROCKET_FLOW) hipLaunchKernelGGL(k_ry_velocity<LB_ROCKET_FLOW>, cells_grid(m.a[0]), dim3(256), 0, fields[0]->stream, m);
    else hipLaunchKernelGGL(k_ry_velocity<LB_ROCKET_FORCES>, cells_grid(m.a[0]), dim3(256), 0, fields[0]->stream, m);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < 2; ++i) fields[i]->feq_valid = false;
    return sc.release();
}

int lb_update_forces_rocket(lb_sim **fields, int count)
{
    int rc = rocket_members(fields, count, "lb_update_forces_rocket");
    if (rc) return rc;
    SetScope sc(fields, 2);
    if ((rc = sc.join())) return rc;
    const RyArgs m = rocket_args(fields);
    if (fields[0]->ry.mode == LB_ROCKET_FLOW) hipLaunchKernelGGL(k_ry_forces<LB_ROCKET_FLOW>, cells_grid(m.a[0]), dim3(256), 0, fields[0]->stream, m);
    else hipLaunchKernelGGL(k_ry_forces<LB_ROCKET_FORCES>, cells_grid(m.a[0]), dim3(256), 0, fields[0]->stream, m);
    HIP_TRY(hipGetLastError());
    return sc.release();
}

int lb_collide_rocket(lb_sim **fields, int count)
{
    int rc = rocket_members(fields, count, "lb_collide_rocket");
    if (rc) return rc;
    for (int i = 0; i < 2; ++i)
        if (!fields[i]->feq) return fail(LB_ERR_STATE, "lb_collide_rocket before lb_update_feq on both members");
    SetScope sc(fields, 2);
    if ((rc = sc.join())) return rc;
    RyArgs m = rocket_args(fields);
    for (int i = 0; i < 2; ++i) m.a[i].dst = fields[i]->origin(fields[i]->cur);      // relaxed in place
    const float *feq_p = fields[0]->feq_origin(), *feq_c = fields[1]->feq_origin();
    if (fields[0]->ry.mode == LB_ROCKET_FLOW) hipLaunchKernelGGL(k_ry_relax<LB_ROCKET_FLOW>, cells_grid(m.a[0]), dim3(256), 0, fields[0]->stream, m, feq_p, feq_c);
    else hipLaunchKernelGGL(k_ry_relax<LB_ROCKET_FORCES>, cells_grid(m.a[0]), dim3(256), 0, fields[0]->stream, m, feq_p, feq_c);
    HIP_TRY(hipGetLastError());
    return sc.release();
}

int lb_get_rocket_fields(lb_sim **fields, int count, float *psi_or_S, float *Fx, float *Fy, float *Fsx, float *Fsy)
{
    int rc = rocket_members(fields, count, "lb_get_rocket_fields");
    if (rc) return rc;
    lb_sim *s = fields[0];
    DeviceGuard guard(s->p.device);
    float *out[5] = {psi_or_S, Fx, Fy, Fsx, Fsy};
    const float *from[5] = {s->ry_op, s->pm_G[0], s->pm_G[1], s->pm_ub[0], s->pm_ub[1]};
    for (int i = 0; i < 5; ++i)
        if (out[i] && (rc = copy_plane_d2h(s, out[i], from[i]))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

}  // extern "C"
