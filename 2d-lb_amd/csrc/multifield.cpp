// multifield.cpp -- coupled scalar lattices (LB_SEM_MULTIFIELD): the kernels of kernels_multifield.h and their launches, the kind's row
// of the kind table (host.h: KindOps) and the set calls lb_run_coupled and lb_collide_coupled.
#include "kernels_multifield.h"    // (first: host.h switches floating-point contraction off for what follows it, cpu_backend.h)
#include "host.h"

namespace {

template <int BC, int NF>
void mf_step_go(bool store_rho, dim3 grid, dim3 block, hipStream_t st, const MfArgs &m)
{
    if (store_rho) hipLaunchKernelGGL((k_mf_step<BC, NF, true>), grid, block, 0, st, m);
    else hipLaunchKernelGGL((k_mf_step<BC, NF, false>), grid, block, 0, st, m);
}

template <int BC>
void mf_step_nf(int nf, bool store_rho, dim3 grid, dim3 block, hipStream_t st, const MfArgs &m)
{
    if (nf == 1) mf_step_go<BC, 1>(store_rho, grid, block, st, m);
    else if (nf == 2) mf_step_go<BC, 2>(store_rho, grid, block, st, m);
    else if (nf == 3) mf_step_go<BC, 3>(store_rho, grid, block, st, m);
    else mf_step_go<BC, 4>(store_rho, grid, block, st, m);
}

// bc: LB_BC_PERIODIC or LB_BC_BOX; nf = 1 ... MF_MAX.  k_mf_step over the whole grid; store_rho: the launch also stores every field's rho.
void mf_step(int bc, int nf, bool store_rho, hipStream_t st, const MfArgs &m)
{
    const StepArgs &a = m.a[0];
    const dim3 block(64, 4), grid = step_grid(a);
    if (bc == LB_BC_PERIODIC) mf_step_nf<LB_BC_PERIODIC>(nf, store_rho, grid, block, st, m);
    else mf_step_nf<LB_BC_BOX>(nf, store_rho, grid, block, st, m);
}

// the un-fused collide_particles of the set: a[i].src relaxed in place towards feq[i], growth from the stored a[i].rho
void mf_collide(int nf, hipStream_t st, const MfArgs &m)
{
    const StepArgs &a = m.a[0];
    const dim3 grid = cells_grid(a), block(256);
    if (nf == 1) hipLaunchKernelGGL(k_mf_collide<1>, grid, block, 0, st, m);
    else if (nf == 2) hipLaunchKernelGGL(k_mf_collide<2>, grid, block, 0, st, m);
    else if (nf == 3) hipLaunchKernelGGL(k_mf_collide<3>, grid, block, 0, st, m);
    else hipLaunchKernelGGL(k_mf_collide<4>, grid, block, 0, st, m);
}

// D2Q9_multifield_fisher.cl's move_bcs: on-node bounce-back on four walls, in place (edge cells only); the periodic family has none
int multifield_move_bcs(lb_sim *s) { return s->p.bc_mode != LB_BC_BOX ? LB_OK : launch_phase(s, grid_edge(s), k_mf_move_bcs, s->origin(s->cur)); }

int multifield_collide(lb_sim *s) { return s->feq ? lb_collide_coupled(&s, 1) : fail(LB_ERR_STATE, "lb_collide_particles before any lb_update_feq"); }

int multifield_run(lb_sim *s, int n_steps) { return lb_run_coupled(&s, 1, n_steps); }

// the members of a set, checked alike for lb_run_coupled and lb_collide_coupled
int coupled_members(lb_sim **f, int count, const char *what)
{
    if (!f || count < 1 || count > MF_MAX) return fail(LB_ERR_ARG, "%s takes 1..%d handles", what, MF_MAX);
    int at = 0;
    switch (set_fault(f, count, LB_SEM_MULTIFIELD, false, true, &at)) {
    case SET_NULL_MEMBER: return fail(LB_ERR_ARG, "null handle in the coupled set");
    case SET_KIND: return fail(LB_ERR_ARG, "the members of a coupled set must be LB_SEM_MULTIFIELD handles");
    case SET_GEOMETRY: return fail(LB_ERR_ARG, "the members of a coupled set must share grid, boundary family, layout flag and device");
    case SET_SPLIT_STEP: return fail(LB_ERR_STATE, "%s inside a split step", what);
    case SET_TWICE: return fail(LB_ERR_ARG, "a handle appears twice in the coupled set");
    default: return LB_OK;
    }
}

}  // namespace

KIND_ROW(kind_multifield,
    "a coupled scalar lattice (LB_SEM_MULTIFIELD)", 1u << LB_BC_PERIODIC | 1u << LB_BC_BOX, "the families LB_BC_PERIODIC and LB_BC_BOX only", false, false,
    0, "a coupled scalar lattice (LB_SEM_MULTIFIELD) takes the variants -1 and 0 only: k_mf_step, no tiles", LB_ERR_ARG,
    nullptr, multifield_move_bcs, scalar_hydro, scalar_feq, multifield_collide, multifield_run)

extern "C" {

int lb_run_coupled(lb_sim **fields, int count, int n_steps)
{
    for (int i = 0; fields && i < count; ++i) NOT_POROUS(fields[i], "lb_run_coupled");
    for (int i = 0; fields && i < count; ++i) NOT_ROCKET(fields[i], "lb_run_coupled");
    int rc = coupled_members(fields, count, "lb_run_coupled");
    if (rc) return rc;
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (n_steps == 0) return LB_OK;
    lb_sim *s0 = fields[0];
    SetScope sc(fields, count);
    if ((rc = sc.join())) return rc;
    for (int it = 0; it < n_steps; ++it) {
        MfArgs m = {};
        for (int i = 0; i < count; ++i) {
            m.a[i] = step_args(fields[i], 0, 1, fields[i]->H);
            m.G[i] = fields[i]->ad_G;
        }
        mf_step(s0->p.bc_mode, count, it == n_steps - 1, s0->stream, m);      // the last launch stores every field's rho
        HIP_TRY(hipGetLastError());
        for (int i = 0; i < count; ++i) fields[i]->cur ^= 1;
    }
    set_ran(fields, count);
    return sc.release();
}

int lb_collide_coupled(lb_sim **fields, int count)
{
    int rc = coupled_members(fields, count, "lb_collide_coupled");
    if (rc) return rc;
    for (int i = 0; i < count; ++i)
        if (!fields[i]->feq) return fail(LB_ERR_STATE, "lb_collide_coupled before lb_update_feq on every member");
    lb_sim *s0 = fields[0];
    SetScope sc(fields, count);
    if ((rc = sc.join())) return rc;
    MfArgs m = {};
    for (int i = 0; i < count; ++i) {
        m.a[i] = step_args(fields[i], 0, 1, fields[i]->H);
        m.a[i].dst = fields[i]->origin(fields[i]->cur);         // relaxed in place
        m.G[i] = fields[i]->ad_G;
        m.feq[i] = fields[i]->feq_origin();
    }
    mf_collide(count, s0->stream, m);
    HIP_TRY(hipGetLastError());
    return sc.release();
}

}  // extern "C"
