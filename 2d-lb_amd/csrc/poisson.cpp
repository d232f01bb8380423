// poisson.cpp -- the translation unit of the LB Poisson solver: instantiates and launches the kernels of kernels_poisson.h
// (poisson_launch.h).
#include "kernels_poisson.h"

namespace {

dim3 cells_grid(const StepArgs &a) { return dim3((unsigned)((a.nx + 255) / 256), (unsigned)a.ny); }
dim3 step_grid(const StepArgs &a) { return dim3((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + 3) / 4)); }

}  // namespace

long long ps_step_blocks(const StepArgs &a)
{
    const dim3 g = step_grid(a);
    return (long long)g.x * g.y;
}

void lbk_ps_step(bool solve, hipStream_t st, const StepArgs &a, const PsExtra &e)
{
    const dim3 block(64, 4), grid = step_grid(a);
    if (solve) hipLaunchKernelGGL(k_ps_step<true>, grid, block, 0, st, a, e);
    else hipLaunchKernelGGL(k_ps_step<false>, grid, block, 0, st, a, e);
}

void lbk_ps_check(hipStream_t st, const float *part, long long blocks, PsState *state, int iter, float tolerance)
{
    hipLaunchKernelGGL(k_ps_check, dim3(1), dim3(PS_CHECK_THREADS), 0, st, part, blocks, state, iter, tolerance);
}

void lbk_ps_gradient(hipStream_t st, const StepArgs &a, float inv_two_dx)
{
    hipLaunchKernelGGL(k_ps_gradient, cells_grid(a), dim3(256), 0, st, a, inv_two_dx);
}

void lbk_ps_move_bcs(hipStream_t st, const StepArgs &a, float *f, float wall)
{
    const int n = a.nx > a.ny ? a.nx : a.ny;
    hipLaunchKernelGGL(k_ps_move_bcs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, f, wall);
}

void lbk_ps_hydro(hipStream_t st, const StepArgs &a) { hipLaunchKernelGGL(k_ps_hydro, cells_grid(a), dim3(256), 0, st, a); }

void lbk_ps_feq(hipStream_t st, const StepArgs &a, float *feq) { hipLaunchKernelGGL(k_ps_feq, cells_grid(a), dim3(256), 0, st, a, feq); }

void lbk_ps_collide(hipStream_t st, const StepArgs &a, float *f, const float *feq, const float *source, float react)
{
    hipLaunchKernelGGL(k_ps_collide, cells_grid(a), dim3(256), 0, st, a, f, feq, source, react);
}
