// advected.cpp -- a flow and the scalars it carries (a dye, a temperature, a growing population under a live velocity field): the kernel
// of kernels_advected.h, its launch, the 1 + NS launch form of the same step and the set call lb_run_advected.  No handle kind and no
// row of the kind table: a set is one whole-grid periodic flow handle (LB_SEM_OPENCL, no obstacles) and 1 ... 2 whole-grid periodic
// scalar lattices (LB_SEM_DIFFUSION) of its grid and device, each with its own omega, growth rate and layout.  Nothing new is
// allocated: lb_destroy has nothing more to free.
#include "kernels_advected.h"   // (first: host.h switches floating-point contraction off for what follows it, cpu_backend.h)
#include "host.h"

namespace {

template <int NS, bool REACT>
void fa_step_go(bool last, dim3 grid, dim3 block, hipStream_t st, const FaArgs &m)
{
    if (last) hipLaunchKernelGGL((k_fa_step<NS, REACT, true>), grid, block, 0, st, m);
    else hipLaunchKernelGGL((k_fa_step<NS, REACT, false>), grid, block, 0, st, m);
}

// k_fa_step over the whole grid; react: some scalar has a growth rate; last: the launch also stores rho, u, v of every member
// (tools/kernel_resources.py advected.cpp k_fa; DESIGN.md has the table)
void fa_step(int ns, bool react, bool last, hipStream_t st, const FaArgs &m)
{
    const dim3 block(64, 4), grid = step_grid(m.flow);
    if (ns == 1) {
        if (react) fa_step_go<1, true>(last, grid, block, st, m);
        else fa_step_go<1, false>(last, grid, block, st, m);
    } else {
        if (react) fa_step_go<2, true>(last, grid, block, st, m);
        else fa_step_go<2, false>(last, grid, block, st, m);
    }
}

// the flow's single-step kernel with its rho, u, v epilogue whatever the handle's flag (launch_step, launch.cpp, leaves the epilogue out
// on a handle that rebuilds the fields on demand: here the scalars read them)
int flow_step_macro(lb_sim *s)
{
    const StepArgs a = step_args(s, 0, 1, s->H);
    const int variant = effective_variant(s);
    const int rpb_sel = variant & LB_VAR_ROWS;
    const int rows_per_block = rpb_sel == LB_VAR_ROWS_1 ? 1 : (rpb_sel == LB_VAR_ROWS_2 ? 2 : 4);
    const dim3 block(64 * (4 / rows_per_block), rows_per_block);
    const dim3 grid((unsigned)((s->pitch / 4 + block.x - 1) / block.x), (unsigned)((s->H + rows_per_block - 1) / rows_per_block));
    lbk_launch_step(LB_BC_PERIODIC, false, true, variant, grid, block, s->stream, a);
    HIP_TRY(hipGetLastError());
    s->cur ^= 1;
    return LB_OK;
}

// the flow and the scalars, checked before anything is enqueued
int advected_members(lb_sim *flow, lb_sim **f, int count, const char *what)
{
    if (!flow) return fail(LB_ERR_ARG, "%s: null flow handle", what);
    if (!f) return fail(LB_ERR_ARG, "%s: null handle array", what);
    if (count < 1 || count > FA_MAX_SCALARS)
        return fail(LB_ERR_ARG, "%s takes 1..%d scalar lattices beside the flow (got a count of %d)", what, FA_MAX_SCALARS, count);
    if (flow->cpu || flow->p.semantics != LB_SEM_OPENCL)
        return fail(LB_ERR_ARG, "%s: the flow is not a GPU flow handle of the OpenCL path (LB_SEM_OPENCL is required)", what);
    if (flow->p.bc_mode != LB_BC_PERIODIC)
        return fail(LB_ERR_ARG, "%s: the flow is not periodic (the family LB_BC_PERIODIC only: the scalar lattice has no wall rule)", what);
    if (flow->multi_slab()) return fail(LB_ERR_STATE, "%s is only available on handles that own the whole grid (the flow is a slab or has LB_FLAG_HALO)", what);
    if (flow->has_mask) return fail(LB_ERR_STATE, "%s: the flow has an obstacle mask (lb_set_mask): the scalar lattice has no obstacle rule", what);
    if (flow->stepping) return fail(LB_ERR_STATE, "%s inside a split step of the flow handle", what);
    for (int i = 0; i < count; ++i) {
        const lb_sim *s = f[i];
        if (!s) return fail(LB_ERR_ARG, "%s: null handle in the set", what);
        if (s->cpu || s->p.semantics != LB_SEM_DIFFUSION)
            return fail(LB_ERR_ARG, "%s: scalar %d is not a scalar lattice on the GPU (LB_SEM_DIFFUSION is required)", what, i);
        for (int j = 0; j < i; ++j)
            if (f[j] == s) return fail(LB_ERR_ARG, "%s: a handle appears twice in the set", what);
        if (s->p.bc_mode != LB_BC_PERIODIC)
            return fail(LB_ERR_ARG, "%s: scalar %d is not periodic (the family LB_BC_PERIODIC only)", what, i);
        if (s->p.nx != flow->p.nx || s->p.ny != flow->p.ny || s->p.device != flow->p.device)
            return fail(LB_ERR_ARG, "%s: scalar %d must have the flow's grid (%d x %d) and device", what, i, flow->p.nx, flow->p.ny);
        if (s->multi_slab()) return fail(LB_ERR_STATE, "%s is only available on handles that own the whole grid", what);
        if (s->stepping) return fail(LB_ERR_STATE, "%s inside a split step", what);
        if (s->ad_Dg != 0.f) return fail(LB_ERR_STATE, "%s: scalar %d has the noisy collision on (lb_set_noise): not built for a carried scalar", what, i);
        if (s->ad_noise_field) return fail(LB_ERR_STATE, "%s: scalar %d holds a noise field (lb_set_noise_field): drop it with NULL first", what, i);
    }
    return LB_OK;
}

}  // namespace

extern "C" {

int lb_run_advected(lb_sim *flow, lb_sim **scalars, int count, int n_steps, int form)
{
    int rc = advected_members(flow, scalars, count, "lb_run_advected");
    if (rc) return rc;
    if (form < -1 || form > 1) return fail(LB_ERR_ARG, "lb_run_advected: form must be -1 (the planner's choice), 0 or 1 (got %d)", form);
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (n_steps == 0) return LB_OK;
    lb_sim *set[1 + FA_MAX_SCALARS] = {flow};
    bool react = false;
    for (int i = 0; i < count; ++i) {
        set[1 + i] = scalars[i];
        react = react || scalars[i]->ad_G != 0.f;
    }
    SetScope sc(set, 1 + count);
    if ((rc = sc.join())) return rc;
    if (advected_form((long long)flow->p.nx * flow->p.ny, count, form) == 1) {
        for (int it = 0; it < n_steps; ++it) {
            FaArgs m = {};
            m.flow = step_args(flow, 0, 1, flow->H);
            for (int i = 0; i < count; ++i) {
                m.s[i] = step_args(scalars[i], 0, 1, scalars[i]->H);
                m.G[i] = scalars[i]->ad_G;
            }
            fa_step(count, react, it == n_steps - 1, flow->stream, m);      // the last launch stores every rho, u, v
            HIP_TRY(hipGetLastError());
            for (int i = 0; i <= count; ++i) set[i]->cur ^= 1;
        }
    } else {
        for (int it = 0; it < n_steps; ++it) {
            if ((rc = flow_step_macro(flow))) return rc;
            for (int i = 0; i < count; ++i)
                if ((rc = scalar_step_carried(scalars[i], flow, it == n_steps - 1))) return rc;
        }
        // the last step's velocity into every scalar's own planes ([H][pitch] whatever the layout of the lattices)
        const long long n4 = flow->pitch * flow->H / 4;
        for (int i = 0; i < count; ++i) {
            if ((rc = copy_quads(flow->stream, scalars[i]->u, flow->u, n4))) return rc;
            if ((rc = copy_quads(flow->stream, scalars[i]->v, flow->v, n4))) return rc;
        }
    }
    set_ran(set, 1 + count);        // (the flow's rho, u, v are stored, as on an eager handle, whatever its flag)
    return sc.release();
}

int lb_advected_kernel(int count, int form, int64_t cells, char *buf, int buflen)
{
    if (!buf || buflen <= 0) return fail(LB_ERR_ARG, "lb_advected_kernel: null buffer");
    if (count < 1 || count > FA_MAX_SCALARS)
        return fail(LB_ERR_ARG, "lb_advected_kernel takes 1..%d scalar lattices beside the flow (got a count of %d)", FA_MAX_SCALARS, count);
    if (form < -1 || form > 1) return fail(LB_ERR_ARG, "lb_advected_kernel: form must be -1 (the planner's choice), 0 or 1 (got %d)", form);
    if (advected_form((long long)cells, count, form) == 1)
        snprintf(buf, (size_t)buflen, "k_fa_step (a flow and the scalars it carries: one launch per step -- pull-stream of all %d lattices, the flow's collide, its u, v in registers, linear-equilibrium collide of each scalar)<NS = %d, PERIODIC>", 1 + count, count);
    else
        snprintf(buf, (size_t)buflen, "k_step<MACRO> + %d x k_ad_step (a flow and the scalars it carries: %d launches per step -- the flow's step stores u, v, each scalar's step reads them from the flow's planes)<PERIODIC>", count, 1 + count);
    return LB_OK;
}

}  // extern "C"
