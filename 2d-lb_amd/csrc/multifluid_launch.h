// multifluid_launch.h -- the seam between multifluid.cpp, which instantiates the kernels of multicomponent Shan-Chen fluids
// (kernels_multifluid.h: LB_SEM_MULTIFLUID), and the host unit that launches them (porous_launch.h does the same for the one fluid
// in a porous medium).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs
#include "porous_launch.h"      // PmExtra: a fluid's G, u_b, force field and constant acceleration (the medium's scalars at epsilon = 1)

constexpr int MC_MAX = 3;           // fluids of a set
constexpr int MC_MAX_INTER = 6;     // entries of its interaction table (lb_interaction, include/lb_hip.h)
constexpr int MC_MAX_REACT = 4;     // entries of its reaction table (lb_fluid_reaction)

struct McInter {
    int i, j, potential;    // fluids; LB_PSI_LINEAR / LB_PSI_SHAN_CHEN / LB_PSI_POW
    float G, par;           // G_int; rho_0 (shan_chen) or alpha (pow)
};
struct McReact {
    int kind, a, b;         // LB_REACT_EAT: eater a, eatee b; LB_REACT_GROW: fluid a
    float p0, p1, p2;       // eat: rate, cutoff, -; grow: min, max, rate
};

// The fluids of a set advanced together: StepArgs as step_args() fills them for each member (a[i].omega its omega, a[i].rho, u, v its
// fields), e[i] as pm_extra() does (G, u_b, field, g, hw), the tables of the set's first handle.  Every fluid's u_b buffers receive
// the same barycentric velocity.
struct McArgs {
    StepArgs a[MC_MAX];
    PmExtra e[MC_MAX];
    McInter inter[MC_MAX_INTER];
    McReact react[MC_MAX_REACT];
    int n_inter, n_react;
};

// bc = LB_BC_PERIODIC or LB_BC_ZERO_GRADIENT; nf = 1 ... MC_MAX.
// The two-launch step: k_mc_moments stores every fluid's post-stream rho, k_mc_collide gathers again, reads rho around the cell,
// and runs forces -> u_b -> feq -> relaxation -> reactions; last: it also stores u, v, G and u_b.
void lbk_mc_moments(int bc, int nf, hipStream_t st, const McArgs &m);
void lbk_mc_collide(int bc, int nf, bool last, hipStream_t st, const McArgs &m);
// The one-launch step k_mc_step: a workgroup owns six rows (three fluids: two) of a 256-cell tile and keeps rho_i of them, of one halo
// row above and below and of one halo cell left and right in LDS; last: it also stores rho, u, v, G and u_b.  Bitwise the two-launch step.
void lbk_mc_step(int bc, int nf, bool last, hipStream_t st, const McArgs &m);
// the un-fused phases: rho, u, v of one fluid from a.src; every fluid's G from the stored rho; u_b from the lattices at a[i].src,
// rho and G; a[i].src relaxed in place towards feq (pm_extra's scalars at epsilon = 1, G a force); the reaction table on a[i].dst in place
void lbk_mc_hydro(hipStream_t st, const StepArgs &a);
void lbk_mc_forces(int bc, int nf, hipStream_t st, const McArgs &m);
void lbk_mc_bary(int nf, hipStream_t st, const McArgs &m);
void lbk_mc_relax(hipStream_t st, const StepArgs &a, const PmExtra &e, float *f, const float *feq);
void lbk_mc_react(int nf, hipStream_t st, const McArgs &m);
