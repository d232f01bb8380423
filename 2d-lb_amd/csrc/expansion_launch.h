// expansion_launch.h -- what the kernels of noisy strains on a shared nutrient (kernels_expansion.h) and the host code that launches
// them (expansion.cpp) share beyond StepArgs.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs

// The members of a set advanced by one launch: StepArgs as step_args() fills them for each member (a[i].omega its omega), the strains
// first, the nutrient behind them.  The imposed velocity every member reads is a[0].u, a[0].v.
constexpr int EX_MAX_STRAINS = 3;
struct ExArgs {
    StepArgs a[EX_MAX_STRAINS + 1];
    const float *edge[EX_MAX_STRAINS + 1];      // OPEN: each member's edge state on the device (scalar_launch.h has the order)
    const float *feq[EX_MAX_STRAINS + 1];       // k_ex_collide only: each member's feq lattice
    float G[EX_MAX_STRAINS], Dg[EX_MAX_STRAINS];        // per strain: growth rate, noise strength (0: nothing is drawn)
    unsigned long long seed[EX_MAX_STRAINS], t[EX_MAX_STRAINS];     // ... its stream's key and the noise counter of this collision
    const float *field[EX_MAX_STRAINS];         // k_ex_collide only: a supplied [ny][nx] field of normals in place of the stream, or nullptr
    float cut;                                  // zero_cutoff
};
