// poisson_launch.h -- the seam between poisson.cpp, which instantiates the kernels of the LB Poisson solver (kernels_poisson.h:
// LB_SEM_POISSON), and the host unit that launches them (scalar_launch.h and multifield_launch.h do the same for their lattices).
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

// workgroups of a k_ps_step launch = partials a k_ps_check folds
long long ps_step_blocks(const StepArgs &a);
// the fused iteration over the whole grid.  solve: the form lb_solve enqueues -- returns at once when the stop word is set, stores rho
// and leaves its workgroup's two sums in e.part; !solve: lb_run's -- no stop word, no sums, rho when e.store_rho
void lbk_ps_step(bool solve, hipStream_t st, const StepArgs &a, const PsExtra &e);
// folds the partials of the k_ps_step in front of it (float64, fixed order), stores the ratio and, if iter >= 2 and the ratio is
// < tolerance (false for inf and NaN), writes iter into the stop word; returns at once when the stop word is set
void lbk_ps_check(hipStream_t st, const float *part, long long blocks, PsState *state, int iter, float tolerance);
// central differences of rho over the box, 0 for a neighbour outside: d/dx into a.u, d/dy into a.v ([H][fpitch], like rho)
void lbk_ps_gradient(hipStream_t st, const StepArgs &a, float inv_two_dx);
// the un-fused phases (lb_move is k_move + copy): move_bcs in place on the lattice at f (edge cells only); rho from a.src; feq from rho;
// f relaxed in place towards feq, plus the source term
void lbk_ps_move_bcs(hipStream_t st, const StepArgs &a, float *f, float wall);
void lbk_ps_hydro(hipStream_t st, const StepArgs &a);
void lbk_ps_feq(hipStream_t st, const StepArgs &a, float *feq);
void lbk_ps_collide(hipStream_t st, const StepArgs &a, float *f, const float *feq, const float *source, float react);
