// porous_launch.h -- the seam between porous.cpp, which instantiates the kernels of forced flow in a porous medium (kernels_porous.h:
// LB_SEM_POROUS), and the host units that launch them (scalar_launch.h, multifield_launch.h and poisson_launch.h do the same for their
// lattices).  Arguments are StepArgs as step_args() fills them for the handle -- src / dst lattices, rho, u, v, layout, nx, ny, omega --
// plus what is below.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs

// The medium and the forces.  Every derived scalar is ONE float32 operation on the host (pm_extra, host.h), so the fused kernel and
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

// the fused step over the whole grid; bc = LB_BC_PERIODIC or LB_BC_ZERO_GRADIENT; last: this launch stores rho, u, v, G and u_b
void lbk_pm_step(int bc, bool last, hipStream_t st, const StepArgs &a, const PmExtra &e);
// the un-fused phases (lb_move is k_move + copy): move_open_bcs in place on the lattice at f (boundary cells only); rho, u, v from
// a.src; G from rho, u, v; u_b from the lattice at f, rho and G; feq from rho and u_b; f relaxed in place towards feq, plus the forcing
void lbk_pm_move_bcs(hipStream_t st, const StepArgs &a, float *f);
void lbk_pm_hydro(hipStream_t st, const StepArgs &a);
void lbk_pm_forces(hipStream_t st, const StepArgs &a, const PmExtra &e);
void lbk_pm_bary(hipStream_t st, const StepArgs &a, const PmExtra &e, const float *f);
void lbk_pm_feq(hipStream_t st, const StepArgs &a, const PmExtra &e, float *feq);
void lbk_pm_collide(hipStream_t st, const StepArgs &a, const PmExtra &e, float *f, const float *feq);
