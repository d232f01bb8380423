// rocket_launch.h -- the seam between rocket.cpp, which instantiates the kernels of surfactant-propelled colonies
// (kernels_rocket.h: LB_SEM_ROCKET), and the host unit that launches them (multifluid_launch.h does the same for the fluids of a
// multicomponent set).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs
#include "plan_consts.h"        // RY_ROWS

// The two lattices of a set advanced together: a[0] the population p, a[1] the surfactant c, StepArgs as step_args() fills them
// (a[i].omega its omega, a[i].rho its density; a[i].u, a[i].v BOTH receive the set's one velocity).  The scalars as ry_args() derives
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

// mode = LB_ROCKET_FLOW or LB_ROCKET_FORCES.
// The two-launch step: k_ry_moments stores both densities, k_ry_collide gathers again, reads the densities around the cell and runs
// stages 3-5; last: it also stores u, v, psi / S and the forces.
void lbk_ry_moments(hipStream_t st, const RyArgs &m);
void lbk_ry_collide(int mode, bool last, hipStream_t st, const RyArgs &m);
// The one-launch step k_ry_step: a workgroup owns RY_ROWS rows of a 256-cell tile and keeps the two stencil operands of them, of one
// halo row above and below and of one halo cell left and right in LDS; last: it also stores rho, u, v, psi / S and the forces.
// Bitwise the two-launch step.
void lbk_ry_step(int mode, bool last, hipStream_t st, const RyArgs &m);
// the un-fused stage 3 and stage 5, from the stored densities: u, v (FLOW: the stencil over rho_c; FORCES: F_p + F_s from the stored
// forces); psi / S and the forces; both lattices at a[i].dst relaxed in place towards feq_p, feq_c
void lbk_ry_velocity(int mode, hipStream_t st, const RyArgs &m);
void lbk_ry_forces(int mode, hipStream_t st, const RyArgs &m);
void lbk_ry_relax(int mode, hipStream_t st, const RyArgs &m, const float *feq_p, const float *feq_c);
