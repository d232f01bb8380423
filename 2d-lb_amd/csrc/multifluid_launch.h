// multifluid_launch.h -- what the kernels of multicomponent Shan-Chen fluids (kernels_multifluid.h: LB_SEM_MULTIFLUID), the host code that
// launches them (multifluid.cpp) and the handle (host.h: the tables of a set) share beyond StepArgs.
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
