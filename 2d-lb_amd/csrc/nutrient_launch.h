// nutrient_launch.h -- what the kernels of a population and its nutrient under a spectral velocity (kernels_nutrient.h) and the host
// code that launches them (nutrient.cpp) share beyond StepArgs.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs

// rows of a 256-cell tile a workgroup of k_sn_step owns: the lane-of-four plan's four waves, each with its own row; the clumpy form
// stages psi of these rows and of one halo row above and below in LDS
constexpr int SN_ROWS = 4;

// The two lattices of a set advanced together: a[0] the population p, a[1] the nutrient n, StepArgs as step_args() fills them
// (a[i].omega its omega, a[i].rho its density; the velocity is read from a[0].u, a[0].v, where the solve has put it).  The scalars as
// nutrient_args() (nutrient.cpp) derives them, every one a single float32 operation there and nowhere else.
struct SnArgs {
    StepArgs a[2];
    float G;                // lb_G: what the population gains and the nutrient loses is w_k G rho_p rho_n
    float inv_cs2;          // float32(1. / (cs * cs)), cs = float32(1 / sqrt(3)), as the reference's kernels form it
    float kf;               // ((-cs) * cs) * G_chen: the factor on the stencil sum
    float rho_o;
    float *psi, *Fx, *Fy;   // [H][pitch] each, with the set's first handle (clumpy only; nullptr until a clumpy call has made them)
};
