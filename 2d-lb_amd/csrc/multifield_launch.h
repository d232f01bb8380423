// multifield_launch.h -- what the kernels of coupled scalar lattices (kernels_multifield.h: LB_SEM_MULTIFIELD) and the host code that
// launches them (multifield.cpp) share beyond StepArgs.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs

// The fields of a coupled set advanced by one launch: StepArgs as step_args() fills them for each member (a[i].omega its omega,
// a[i].corner its corner state: the eight never-written corner links of LB_BC_BOX in the ABI's order, include/lb_hip.h), its
// growth rate and -- k_mf_collide only -- its feq lattice.  The imposed velocity every field reads is a[0].u, a[0].v.
constexpr int MF_MAX = 4;
struct MfArgs {
    StepArgs a[MF_MAX];
    float G[MF_MAX];
    const float *feq[MF_MAX];
};
