// expansion.cpp -- noisy strains on a shared nutrient (the reference's advecting_range_expansion/stochastic_nutrients.py): the kernels of
// kernels_expansion.h, their launches and the set calls lb_run_expansion, lb_update_hydro_expansion and lb_collide_expansion.  No handle
// kind and no row of the kind table: a set is 2 ... 4 whole-grid scalar lattices (LB_SEM_DIFFUSION) of one family, LB_BC_OPEN or
// LB_BC_PERIODIC -- the strains first, the nutrient last.  A strain's growth rate and noise are its handle's (lb_set_reaction,
// lb_set_noise); zero_cutoff travels with every call.  Nothing new is allocated: lb_destroy has nothing more to free.
#include "kernels_expansion.h"  // (first: host.h switches floating-point contraction off for what follows it, cpu_backend.h)
#include "host.h"

namespace {

template <int BC, int NP>
void ex_step_go(bool store_rho, dim3 grid, dim3 block, hipStream_t st, const ExArgs &m)
{
    if (store_rho) hipLaunchKernelGGL((k_ex_step<BC, NP, true>), grid, block, 0, st, m);
    else hipLaunchKernelGGL((k_ex_step<BC, NP, false>), grid, block, 0, st, m);
}

template <int BC>
void ex_step_np(int np, bool store_rho, dim3 grid, dim3 block, hipStream_t st, const ExArgs &m)
{
    if (np == 1) ex_step_go<BC, 1>(store_rho, grid, block, st, m);
    else if (np == 2) ex_step_go<BC, 2>(store_rho, grid, block, st, m);
    else ex_step_go<BC, 3>(store_rho, grid, block, st, m);
}

// bc: LB_BC_PERIODIC or LB_BC_OPEN; np = 1 ... EX_MAX_STRAINS.  k_ex_step over the whole grid; store_rho: the launch also stores every
// member's cut rho (tools/kernel_resources.py expansion.cpp k_ex; DESIGN.md has the table)
void ex_step(int bc, int np, bool store_rho, hipStream_t st, const ExArgs &m)
{
    const dim3 block(64, 4), grid = step_grid(m.a[0]);
    if (bc == LB_BC_PERIODIC) ex_step_np<LB_BC_PERIODIC>(np, store_rho, grid, block, st, m);
    else ex_step_np<LB_BC_OPEN>(np, store_rho, grid, block, st, m);
}

// the members of a set and the parameters, checked alike for every set call
int expansion_members(lb_sim **f, int count, const lb_expansion_params *p, const char *what)
{
    if (!f) return fail(LB_ERR_ARG, "%s: null handle array", what);
    if (!p) return fail(LB_ERR_ARG, "%s: null parameters", what);
    if (count < 2 || count > EX_MAX_STRAINS + 1)
        return fail(LB_ERR_ARG, "%s takes 2..%d handles, 1..%d strains and the nutrient behind them (got a count of %d)", what,
                    EX_MAX_STRAINS + 1, EX_MAX_STRAINS, count);
    // (not set_fault's order: the family stands between the kind and the shared geometry, the split step behind the parameters)
    for (int i = 0; i < count; ++i) {
        lb_sim *s = f[i];
        if (!s) return fail(LB_ERR_ARG, "%s: null handle in the set", what);
        NOT_ROCKET(s, what);
        if (s->cpu || s->p.semantics != LB_SEM_DIFFUSION)
            return fail(LB_ERR_ARG, "%s: handle %d is not a scalar lattice on the GPU (LB_SEM_DIFFUSION is required)", what, i);
        for (int j = 0; j < i; ++j)
            if (f[j] == s) return fail(LB_ERR_ARG, "%s: a handle appears twice in the set", what);
        if (s->p.bc_mode != LB_BC_OPEN && s->p.bc_mode != LB_BC_PERIODIC)
            return fail(LB_ERR_ARG, "%s: handle %d is neither open nor periodic (the families LB_BC_OPEN and LB_BC_PERIODIC only)", what, i);
        if (!same_geometry(s, f[0]))
            return fail(LB_ERR_ARG, "%s: the strains and the nutrient must share grid (geometry), boundary family, layout flag and device", what);
    }
    if (!finite32(p->zero_cutoff)) return fail(LB_ERR_ARG, "%s: zero_cutoff must be finite", what);
    const lb_sim *nut = f[count - 1];
    if (nut->ad_G != 0.f) return fail(LB_ERR_ARG, "%s: the nutrient (the last handle) has a growth rate (lb_set_reaction): it must be 0", what);
    for (int i = 0; i + 1 < count; ++i)
        for (int j = 0; j < i; ++j)
            if (f[i]->ad_Dg != 0.f && f[j]->ad_Dg != 0.f && f[i]->ad_seed == f[j]->ad_seed)
                return fail(LB_ERR_ARG, "%s: the noisy strains %d and %d have the same seed: they would draw the same normals", what, j, i);
    for (int i = 0; i < count; ++i) {
        if (f[i]->multi_slab()) return fail(LB_ERR_STATE, "%s is only available on handles that own the whole grid", what);
        if (f[i]->stepping) return fail(LB_ERR_STATE, "%s inside a split step", what);
    }
    if (nut->ad_Dg != 0.f) return fail(LB_ERR_STATE, "%s: the nutrient (the last handle) has the noisy collision on (lb_set_noise): only strains draw", what);
    return LB_OK;
}

// (src = the current lattice, dst = the other one: what the fused step reads and writes; the collision stage sets dst itself)
ExArgs expansion_args(lb_sim **f, int count, const lb_expansion_params &p)
{
    ExArgs m = {};
    for (int i = 0; i < count; ++i) {
        m.a[i] = step_args(f[i], 0, 1, f[i]->H);
        m.edge[i] = f[i]->ad_edge;
    }
    for (int i = 0; i + 1 < count; ++i) {
        m.G[i] = f[i]->ad_G;
        m.Dg[i] = f[i]->ad_Dg;
        m.seed[i] = f[i]->ad_seed;
        m.t[i] = f[i]->ad_t;
    }
    m.cut = p.zero_cutoff;
    return m;
}

}  // namespace

extern "C" {

int lb_run_expansion(lb_sim **fields, int count, const lb_expansion_params *p, int n_steps)
{
    int rc = expansion_members(fields, count, p, "lb_run_expansion");
    if (rc) return rc;
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    for (int i = 0; i < count; ++i)
        if (fields[i]->ad_noise_field)
            return fail(LB_ERR_STATE, "lb_run_expansion: handle %d holds a noise field (lb_set_noise_field): only lb_collide_expansion uses one; drop it with NULL first", i);
    if (n_steps == 0) return LB_OK;
    lb_sim *s0 = fields[0];
    SetScope sc(fields, count);
    if ((rc = sc.join())) return rc;
    for (int it = 0; it < n_steps; ++it) {
        ex_step(s0->p.bc_mode, count - 1, it == n_steps - 1, s0->stream, expansion_args(fields, count, *p));     // the last launch stores every rho
        HIP_TRY(hipGetLastError());
        for (int i = 0; i < count; ++i) {
            fields[i]->cur ^= 1;
            if (i + 1 < count && fields[i]->ad_Dg != 0.f) fields[i]->ad_t += 1;
        }
    }
    set_ran(fields, count);
    return sc.release();
}

int lb_update_hydro_expansion(lb_sim **fields, int count, const lb_expansion_params *p)
{
    int rc = expansion_members(fields, count, p, "lb_update_hydro_expansion");
    if (rc) return rc;
    lb_sim *s0 = fields[0];
    SetScope sc(fields, count);
    if ((rc = sc.join())) return rc;
    const ExArgs m = expansion_args(fields, count, *p);
    const dim3 grid = cells_grid(m.a[0]), block(256);
    if (count == 2) hipLaunchKernelGGL(k_ex_hydro<2>, grid, block, 0, s0->stream, m);
    else if (count == 3) hipLaunchKernelGGL(k_ex_hydro<3>, grid, block, 0, s0->stream, m);
    else hipLaunchKernelGGL(k_ex_hydro<4>, grid, block, 0, s0->stream, m);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < count; ++i) fields[i]->macro_valid = true;      // (feq keeps its previous content, as after lb_update_hydro)
    return sc.release();
}

int lb_collide_expansion(lb_sim **fields, int count, const lb_expansion_params *p)
{
    int rc = expansion_members(fields, count, p, "lb_collide_expansion");
    if (rc) return rc;
    for (int i = 0; i < count; ++i)
        if (!fields[i]->feq) return fail(LB_ERR_STATE, "lb_collide_expansion before lb_update_feq on every member");
    lb_sim *s0 = fields[0];
    SetScope sc(fields, count);
    if ((rc = sc.join())) return rc;
    ExArgs m = expansion_args(fields, count, *p);
    for (int i = 0; i < count; ++i) {
        m.a[i].dst = fields[i]->origin(fields[i]->cur);         // relaxed in place
        m.feq[i] = fields[i]->feq_origin();
        if (i + 1 < count) m.field[i] = fields[i]->ad_noise_field;
    }
    const dim3 grid = cells_grid(m.a[0]), block(256);
    if (count == 2) hipLaunchKernelGGL(k_ex_collide<1>, grid, block, 0, s0->stream, m);
    else if (count == 3) hipLaunchKernelGGL(k_ex_collide<2>, grid, block, 0, s0->stream, m);
    else hipLaunchKernelGGL(k_ex_collide<3>, grid, block, 0, s0->stream, m);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i + 1 < count; ++i)
        if (fields[i]->ad_Dg != 0.f) fields[i]->ad_t += 1;      // one noisy collision, from the stream or the supplied field
    return sc.release();
}

}  // extern "C"
