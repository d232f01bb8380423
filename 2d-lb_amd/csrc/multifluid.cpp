// multifluid.cpp -- multicomponent Shan-Chen fluids (LB_SEM_MULTIFLUID): the kernels of kernels_multifluid.h and their launches, the
// kind's row of the kind table (host.h: KindOps) and the set calls: lb_run_fluids, the tables of a set, the un-fused stages.
#include "kernels_multifluid.h"    // (first: host.h switches floating-point contraction off for what follows it, cpu_backend.h)
#include "host.h"

namespace {

template <int BC, int NF>
void launch_moments(hipStream_t st, const McArgs &m)
{
    hipLaunchKernelGGL((k_mc_moments<BC, NF>), step_grid(m.a[0]), dim3(64, 4), 0, st, m);
}

template <int BC, int NF>
void launch_collide(bool last, hipStream_t st, const McArgs &m)
{
    if (last) hipLaunchKernelGGL((k_mc_collide<BC, NF, true>), step_grid(m.a[0]), dim3(64, 4), 0, st, m);
    else hipLaunchKernelGGL((k_mc_collide<BC, NF, false>), step_grid(m.a[0]), dim3(64, 4), 0, st, m);
}

// rows a workgroup of k_mc_step owns: six (eight waves, two per SIMD: at most 256 registers each) for one and two fluids; two (four
// waves, one per SIMD) for three, whose cell does not fit 256 registers (tools/kernel_resources.py multifluid.cpp k_mc)
template <int NF>
constexpr int step_rows() { return NF == 3 ? 2 : 6; }

template <int BC, int NF>
void launch_fused(bool last, hipStream_t st, const McArgs &m)
{
    constexpr int R = step_rows<NF>();
    const StepArgs &a = m.a[0];
    const dim3 grid((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + R - 1) / R)), block(64, R + 2);
    if (last) hipLaunchKernelGGL((k_mc_step<BC, NF, R, true>), grid, block, 0, st, m);
    else hipLaunchKernelGGL((k_mc_step<BC, NF, R, false>), grid, block, 0, st, m);
}

template <int BC, int NF>
void launch_forces(hipStream_t st, const McArgs &m)
{
    hipLaunchKernelGGL((k_mc_forces<BC, NF>), cells_grid(m.a[0]), dim3(256), 0, st, m);
}

// f<BC, NF>(args...) for the run-time bc and nf
#define MC_DISPATCH(f, ...)                                                 \
    do {                                                                    \
        if (bc == LB_BC_PERIODIC) {                                         \
            if (nf == 1) f<LB_BC_PERIODIC, 1>(__VA_ARGS__);                 \
            else if (nf == 2) f<LB_BC_PERIODIC, 2>(__VA_ARGS__);            \
            else f<LB_BC_PERIODIC, 3>(__VA_ARGS__);                         \
        } else {                                                            \
            if (nf == 1) f<LB_BC_ZERO_GRADIENT, 1>(__VA_ARGS__);            \
            else if (nf == 2) f<LB_BC_ZERO_GRADIENT, 2>(__VA_ARGS__);       \
            else f<LB_BC_ZERO_GRADIENT, 3>(__VA_ARGS__);                    \
        }                                                                   \
    } while (0)

// bc = LB_BC_PERIODIC or LB_BC_ZERO_GRADIENT; nf = 1 ... MC_MAX.
// The two-launch step: k_mc_moments stores every fluid's post-stream rho, k_mc_collide gathers again, reads rho around the cell,
// and runs forces -> u_b -> feq -> relaxation -> reactions; last: it also stores u, v, G and u_b.
void mc_moments(int bc, int nf, hipStream_t st, const McArgs &m) { MC_DISPATCH(launch_moments, st, m); }
void mc_collide(int bc, int nf, bool last, hipStream_t st, const McArgs &m) { MC_DISPATCH(launch_collide, last, st, m); }
// The one-launch step k_mc_step: a workgroup owns six rows (three fluids: two) of a 256-cell tile and keeps rho_i of them, of one halo
// row above and below and of one halo cell left and right in LDS; last: it also stores rho, u, v, G and u_b.  Bitwise the two-launch step.
void mc_step(int bc, int nf, bool last, hipStream_t st, const McArgs &m) { MC_DISPATCH(launch_fused, last, st, m); }
// the un-fused stages: every fluid's G from the stored rho; u_b from the lattices at a[i].src, rho and G; the reaction table on a[i].dst in place
void mc_forces(int bc, int nf, hipStream_t st, const McArgs &m) { MC_DISPATCH(launch_forces, st, m); }

void mc_bary(int nf, hipStream_t st, const McArgs &m)
{
    const dim3 grid = cells_grid(m.a[0]);
    if (nf == 1) hipLaunchKernelGGL(k_mc_bary<1>, grid, dim3(256), 0, st, m);
    else if (nf == 2) hipLaunchKernelGGL(k_mc_bary<2>, grid, dim3(256), 0, st, m);
    else hipLaunchKernelGGL(k_mc_bary<3>, grid, dim3(256), 0, st, m);
}

void mc_react(int nf, hipStream_t st, const McArgs &m)
{
    const dim3 grid = cells_grid(m.a[0]);
    if (nf == 1) hipLaunchKernelGGL(k_mc_react<1>, grid, dim3(256), 0, st, m);
    else if (nf == 2) hipLaunchKernelGGL(k_mc_react<2>, grid, dim3(256), 0, st, m);
    else hipLaunchKernelGGL(k_mc_react<3>, grid, dim3(256), 0, st, m);
}

int multifluid_hydro(lb_sim *s) { return launch_phase(s, grid_cells(s), k_mc_hydro); }   // rho, and u, v where rho > 1e-12

// f relaxed in place towards feq (pm_extra's scalars at epsilon = 1, G a force)
int multifluid_collide(lb_sim *s)
{
    int rc = collide_ready(s);
    return rc ? rc : launch_phase(s, grid_cells(s), k_mc_relax, pm_extra(s), s->origin(s->cur), s->feq_origin());
}

int multifluid_run(lb_sim *s, int n_steps) { return lb_run_fluids(&s, 1, n_steps); }

// the members of a set, checked alike for every set call
int fluid_members(lb_sim **f, int count, const char *what)
{
    if (!f) return fail(LB_ERR_ARG, "%s: null handle array", what);
    if (count < 1 || count > MC_MAX) return fail(LB_ERR_ARG, "%s takes 1..%d handles (more than %d fluids are not built)", what, MC_MAX, MC_MAX);
    int at = 0;
    switch (set_fault(f, count, LB_SEM_MULTIFLUID, true, false, &at)) {
    case SET_NULL_MEMBER: return fail(LB_ERR_ARG, "null handle in the set of fluids");
    case SET_ROCKET_NAMED: return ROCKET_REFUSED(what);
    case SET_KIND: return fail(LB_ERR_STATE, "%s is for the fluids of a multicomponent set (LB_SEM_MULTIFLUID)", what);
    case SET_GEOMETRY: return fail(LB_ERR_ARG, "the fluids of a set must share grid, boundary family, layout flag and device (fluids of different families in one set are not built)");
    case SET_TWICE: return fail(LB_ERR_ARG, "a handle appears twice in the set of fluids");
    default: break;
    }
    // the tables name fluids by their place in the set
    for (int t = 0; t < f[0]->mc_n_inter; ++t)
        if (f[0]->mc_inter[t].i >= count || f[0]->mc_inter[t].j >= count)
            return fail(LB_ERR_STATE, "%s: the interaction table of the first handle names fluid %d of a set of %d", what,
                        f[0]->mc_inter[t].i > f[0]->mc_inter[t].j ? f[0]->mc_inter[t].i : f[0]->mc_inter[t].j, count);
    for (int t = 0; t < f[0]->mc_n_react; ++t)
        if (f[0]->mc_react[t].a >= count || f[0]->mc_react[t].b >= count)
            return fail(LB_ERR_STATE, "%s: the reaction table of the first handle names a fluid outside a set of %d", what, count);
    return LB_OK;
}

// (src = dst = the current lattice: what the phases read and write in place; the two-launch step sets dst itself)
McArgs fluid_args(lb_sim **f, int count)
{
    McArgs m = {};
    for (int i = 0; i < count; ++i) {
        m.a[i] = step_args(f[i], 0, 1, f[i]->H);
        m.e[i] = pm_extra(f[i]);
    }
    for (int t = 0; t < f[0]->mc_n_inter; ++t) m.inter[t] = f[0]->mc_inter[t];
    for (int t = 0; t < f[0]->mc_n_react; ++t) m.react[t] = f[0]->mc_react[t];
    m.n_inter = f[0]->mc_n_inter;
    m.n_react = f[0]->mc_n_react;
    return m;
}

}  // namespace

KIND_ROW(kind_multifluid,
    "a fluid of a multicomponent set (LB_SEM_MULTIFLUID)", 1u << LB_BC_PERIODIC | 1u << LB_BC_ZERO_GRADIENT, "the families LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT only", true, true,
    1, "lb_set_variant: a fluid of a multicomponent set (LB_SEM_MULTIFLUID) takes the variants -1 (the planner's choice), 0 (the two-launch step k_mc_moments + k_mc_collide) and 1 (the one-launch step k_mc_step) only", LB_ERR_STATE,
    forced_create, porous_move_bcs, multifluid_hydro, porous_feq, multifluid_collide, multifluid_run)

extern "C" {

int lb_run_fluids(lb_sim **fluids, int count, int n_steps)
{
    int rc = fluid_members(fluids, count, "lb_run_fluids");
    if (rc) return rc;
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (n_steps == 0) return LB_OK;
    lb_sim *s0 = fluids[0];
    SetScope sc(fluids, count);
    if ((rc = sc.join())) return rc;
    for (int it = 0; it < n_steps; ++it) {
        const McArgs m = fluid_args(fluids, count);
        if (multifluid_one_launch(s0)) {            // (the set's first handle chooses: lb_set_variant; plan.cpp)
            mc_step(s0->p.bc_mode, count, it == n_steps - 1, s0->stream, m);        // the last one stores rho, u, v, G and u_b
            HIP_TRY(hipGetLastError());
        } else {
            mc_moments(s0->p.bc_mode, count, s0->stream, m);
            HIP_TRY(hipGetLastError());
            mc_collide(s0->p.bc_mode, count, it == n_steps - 1, s0->stream, m);     // the last one stores u, v, G and u_b
            HIP_TRY(hipGetLastError());
        }
        for (int i = 0; i < count; ++i) fluids[i]->cur ^= 1;
    }
    set_ran(fluids, count);
    return sc.release();
}

int lb_set_interactions(lb_sim **fluids, int count, const lb_interaction *table, int n)
{
    int rc = fluid_members(fluids, count, "lb_set_interactions");
    if (rc) return rc;
    if (n < 0 || n > MC_MAX_INTER || (n > 0 && !table)) return fail(LB_ERR_ARG, "lb_set_interactions takes 0..%d entries", MC_MAX_INTER);
    McInter in[MC_MAX_INTER] = {};
    for (int t = 0; t < n; ++t) {
        const lb_interaction &e = table[t];
        if (e.fluid_1 < 0 || e.fluid_1 >= count || e.fluid_2 < 0 || e.fluid_2 >= count)
            return fail(LB_ERR_ARG, "interaction %d names fluids %d and %d of a set of %d", t, e.fluid_1, e.fluid_2, count);
        if (e.potential != LB_PSI_LINEAR && e.potential != LB_PSI_SHAN_CHEN && e.potential != LB_PSI_POW)
            return fail(LB_ERR_ARG, "interaction %d: unknown potential %d (linear, shan_chen and pow are built; vdw is not)", t, e.potential);
        if (e.boundary != (fluids[0]->p.bc_mode == LB_BC_PERIODIC ? 0 : 1))
            return fail(LB_ERR_ARG, "interaction %d: the stencil's boundary rule (%d) must be the set's family (%s)", t, e.boundary,
                        fluids[0]->p.bc_mode == LB_BC_PERIODIC ? "0, periodic" : "1, zero gradient");
        if (!finite32(e.G_int) || !finite32(e.parameter)) return fail(LB_ERR_ARG, "interaction %d: G_int and the parameter must be finite", t);
        if (e.potential == LB_PSI_SHAN_CHEN && e.parameter == 0.f) return fail(LB_ERR_ARG, "interaction %d: shan_chen needs rho_0 != 0", t);
        in[t] = McInter{e.fluid_1, e.fluid_2, e.potential, e.G_int, e.parameter};
    }
    for (int t = 0; t < MC_MAX_INTER; ++t) fluids[0]->mc_inter[t] = in[t];
    fluids[0]->mc_n_inter = n;
    return LB_OK;
}

int lb_set_reactions(lb_sim **fluids, int count, const lb_fluid_reaction *table, int n)
{
    int rc = fluid_members(fluids, count, "lb_set_reactions");
    if (rc) return rc;
    if (n < 0 || n > MC_MAX_REACT || (n > 0 && !table)) return fail(LB_ERR_ARG, "lb_set_reactions takes 0..%d entries", MC_MAX_REACT);
    McReact re[MC_MAX_REACT] = {};
    for (int t = 0; t < n; ++t) {
        const lb_fluid_reaction &e = table[t];
        if (e.kind != LB_REACT_EAT && e.kind != LB_REACT_GROW) return fail(LB_ERR_ARG, "reaction %d: unknown kind %d", t, e.kind);
        if (e.fluid_a < 0 || e.fluid_a >= count) return fail(LB_ERR_ARG, "reaction %d names fluid %d of a set of %d", t, e.fluid_a, count);
        if (e.kind == LB_REACT_EAT && (e.fluid_b < 0 || e.fluid_b >= count || e.fluid_b == e.fluid_a))
            return fail(LB_ERR_ARG, "reaction %d: the eatee must be another fluid of the set (got %d, eater %d)", t, e.fluid_b, e.fluid_a);
        if (!finite32(e.p0) || !finite32(e.p1) || !finite32(e.p2)) return fail(LB_ERR_ARG, "reaction %d: the parameters must be finite", t);
        re[t] = McReact{e.kind, e.fluid_a, e.kind == LB_REACT_EAT ? e.fluid_b : 0, e.p0, e.p1, e.p2};
    }
    for (int t = 0; t < MC_MAX_REACT; ++t) fluids[0]->mc_react[t] = re[t];
    fluids[0]->mc_n_react = n;
    return LB_OK;
}

int lb_get_interactions(lb_sim *first, lb_interaction *table, int *n)
{
    if (!first) return fail(LB_ERR_ARG, "null handle");
    NOT_ROCKET(first, "lb_get_interactions");
    if (first->cpu || !first->multifluid()) return fail(LB_ERR_STATE, "lb_get_interactions is for the fluids of a multicomponent set (LB_SEM_MULTIFLUID)");
    if (n) *n = first->mc_n_inter;
    for (int t = 0; table && t < first->mc_n_inter; ++t) {
        const McInter &e = first->mc_inter[t];
        table[t] = lb_interaction{e.i, e.j, e.potential, first->p.bc_mode == LB_BC_PERIODIC ? 0 : 1, e.G, e.par};
    }
    return LB_OK;
}

int lb_get_reactions(lb_sim *first, lb_fluid_reaction *table, int *n)
{
    if (!first) return fail(LB_ERR_ARG, "null handle");
    NOT_ROCKET(first, "lb_get_reactions");
    if (first->cpu || !first->multifluid()) return fail(LB_ERR_STATE, "lb_get_reactions is for the fluids of a multicomponent set (LB_SEM_MULTIFLUID)");
    if (n) *n = first->mc_n_react;
    for (int t = 0; table && t < first->mc_n_react; ++t) {
        const McReact &e = first->mc_react[t];
        table[t] = lb_fluid_reaction{e.kind, e.a, e.b, e.p0, e.p1, e.p2};
    }
    return LB_OK;
}

int lb_update_forces_fluids(lb_sim **fluids, int count)
{
    int rc = fluid_members(fluids, count, "lb_update_forces_fluids");
    if (rc) return rc;
    SetScope sc(fluids, count);
    if ((rc = sc.join())) return rc;
    mc_forces(fluids[0]->p.bc_mode, count, fluids[0]->stream, fluid_args(fluids, count));
    HIP_TRY(hipGetLastError());
    return sc.release();
}

int lb_update_bary_fluids(lb_sim **fluids, int count)
{
    int rc = fluid_members(fluids, count, "lb_update_bary_fluids");
    if (rc) return rc;
    SetScope sc(fluids, count);
    if ((rc = sc.join())) return rc;
    mc_bary(count, fluids[0]->stream, fluid_args(fluids, count));
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < count; ++i) fluids[i]->feq_valid = false;
    return sc.release();
}

int lb_react_fluids(lb_sim **fluids, int count)
{
    int rc = fluid_members(fluids, count, "lb_react_fluids");
    if (rc) return rc;
    if (fluids[0]->mc_n_react == 0) return LB_OK;
    SetScope sc(fluids, count);
    if ((rc = sc.join())) return rc;
    McArgs m = fluid_args(fluids, count);
    for (int i = 0; i < count; ++i) m.a[i].dst = fluids[i]->origin(fluids[i]->cur);       // in place
    mc_react(count, fluids[0]->stream, m);
    HIP_TRY(hipGetLastError());
    return sc.release();
}

}  // extern "C"
