// porous_launch.h -- what the kernels of forced flow in a porous medium (kernels_porous.h: LB_SEM_POROUS) and the host code that launches
// them (porous.cpp; multifluid.cpp for a fluid of a set) share beyond StepArgs.  Arguments are StepArgs as step_args() fills them for the handle -- src / dst lattices, rho, u, v, layout, nx, ny, omega --
// plus what is below.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs

// The medium and the forces.  Every derived scalar is ONE float32 operation on the host (pm_extra, porous.cpp), so the fused kernel and
// the phases are handed the same bits.
struct PmExtra {
    float *Gx, *Gy;             // [H][fpitch]: the total force of the last step (stage 5's output)
    float *ub, *vb;             // [H][fpitch]: the barycentric velocity (stage 6's output; lb_set_bary_velocity)
    const float *fgx, *fgy;     // [H][fpitch]: the force field, or nullptr
    float gx, gy;               // the sum of the constant forces
    float eps;                  // epsilon
    float en, ef;               // epsilon nu_fluid, epsilon Fe
    float K, sqrtK;             // K, sqrtf(K)
    float a15, a45;             // 1.5 / epsilon, 4.5 / epsilon    (as 1.5f * (1.f / eps), ...)
    float b3, b9;               // 3 / epsilon, 9 / epsilon
    float hw;                   // 1 - omega / 2
};
