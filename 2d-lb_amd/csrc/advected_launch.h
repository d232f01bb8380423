// advected_launch.h -- what the kernel of a flow and the scalars it carries (kernels_advected.h) and the host code that launches it
// (advected.cpp) share beyond StepArgs.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs

// The lattices advanced by one launch: StepArgs as step_args() fills them, the flow's and one per scalar (s[i].omega its omega, G[i] its
// growth rate).  The geometry is the flow's; a member's pitch and plane stride are its own (LB_FLAG_PLANAR on any of them).
constexpr int FA_MAX_SCALARS = 2;
struct FaArgs {
    StepArgs flow;
    StepArgs s[FA_MAX_SCALARS];
    float G[FA_MAX_SCALARS];
};
