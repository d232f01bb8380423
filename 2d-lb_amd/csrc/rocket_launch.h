// rocket_launch.h -- what the kernels of surfactant-propelled colonies (kernels_rocket.h: LB_SEM_ROCKET) and the host code that launches
// them (rocket.cpp) share beyond StepArgs.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs
#include "plan_consts.h"        // RY_ROWS

// The two lattices of a set advanced together: a[0] the population p, a[1] the surfactant c, StepArgs as step_args() fills them
// (a[i].omega its omega, a[i].rho its density; a[i].u, a[i].v BOTH receive the set's one velocity).  The scalars as rocket_args() (rocket.cpp) derives
// them, every one a single float32 operation there and nowhere else.
struct RyArgs {
    StepArgs a[2];
    float G, Gc;            // lb_G, lb_Gc: the population's growth rate and the surfactant's secretion rate
    float inv_cs2;          // float32(1. / (cs * cs)), cs = float32(1 / sqrt(3)), as the reference's kernels form it
    float ke;               // (-epsilon) * inv_cs2
    float ngc;              // -G_chen
    float rho_o, c_o, alpha;
    float *op;              // [H][pitch]: psi (LB_ROCKET_FLOW) / S (LB_ROCKET_FORCES)
    float *Fx, *Fy;         // the pseudo-force F (FLOW) / the pressure force F_p (FORCES)
    float *Sx, *Sy;         // the surface force F_s (FORCES only)
};
