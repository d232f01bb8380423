// poisson_launch.h -- what the kernels of the LB Poisson solver (kernels_poisson.h: LB_SEM_POISSON), the host code that launches them
// (poisson.cpp) and the handle (host.h: PsState) share beyond StepArgs.
// Arguments are StepArgs as step_args() fills them for the handle -- src / dst lattices, rho (the PREVIOUS iteration's on entry, this
// one's on exit), layout, nx, ny, omega, corner (the eight never-written corner links, in LB_BC_BOX's order) -- plus what is below.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs

// What the device keeps of a solve (one per handle, 16 bytes): written by k_ps_check with ordinary vector stores, read by every
// k_ps_step<true> / k_ps_check as their first instruction, and by the host once per batch of launches (the stop word alone).
struct PsState {
    int stop;           // 0, or the iteration index (since the last lb_solve_reset) at which the run converged
    float ratio;        // mean |rho - rho_before| / mean rho_before of the last iteration checked
    int ratio_iter;     // ... and that iteration's index (0: none yet)
    int pad;
};

struct PsExtra {
    const float *source;    // [H][fpitch]: the scaled source (padding zero)
    float *part;            // two floats per workgroup of k_ps_step: sum |rho_new - rho_old|, sum rho_old over its cells inside the box
    const PsState *state;
    float wall;             // (w0 - 1) rho_on_boundary, one float32 product
    float react;            // delta_t D of collide_particles: react = source x this
    int store_rho;          // k_ps_step<false>: this launch stores rho (the last of an lb_run)
};

// workgroups of a k_ps_step launch = partials a k_ps_check folds (poisson.cpp)
long long ps_step_blocks(const StepArgs &a);
