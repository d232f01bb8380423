// porous.cpp -- the translation unit of forced flow in a porous medium: instantiates and launches the kernels of kernels_porous.h
// (porous_launch.h).
#include "kernels_porous.h"

namespace {

dim3 cells_grid(const StepArgs &a) { return dim3((unsigned)((a.nx + 255) / 256), (unsigned)a.ny); }
dim3 step_grid(const StepArgs &a) { return dim3((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + 3) / 4)); }

template <int BC>
void launch_step(bool field, bool last, hipStream_t st, const StepArgs &a, const PmExtra &e)
{
    const dim3 block(64, 4), grid = step_grid(a);
    if (field) {
        if (last) hipLaunchKernelGGL((k_pm_step<BC, true, true>), grid, block, 0, st, a, e);
        else hipLaunchKernelGGL((k_pm_step<BC, true, false>), grid, block, 0, st, a, e);
    } else {
        if (last) hipLaunchKernelGGL((k_pm_step<BC, false, true>), grid, block, 0, st, a, e);
        else hipLaunchKernelGGL((k_pm_step<BC, false, false>), grid, block, 0, st, a, e);
    }
}

}  // namespace

void lbk_pm_step(int bc, bool last, hipStream_t st, const StepArgs &a, const PmExtra &e)
{
    if (bc == LB_BC_PERIODIC) launch_step<LB_BC_PERIODIC>(e.fgx != nullptr, last, st, a, e);
    else launch_step<LB_BC_ZERO_GRADIENT>(e.fgx != nullptr, last, st, a, e);
}

void lbk_pm_move_bcs(hipStream_t st, const StepArgs &a, float *f)
{
    const int n = a.nx > a.ny ? a.nx : a.ny;
    hipLaunchKernelGGL(k_pm_move_bcs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, f);
}

void lbk_pm_hydro(hipStream_t st, const StepArgs &a) { hipLaunchKernelGGL(k_pm_hydro, cells_grid(a), dim3(256), 0, st, a); }

void lbk_pm_forces(hipStream_t st, const StepArgs &a, const PmExtra &e) { hipLaunchKernelGGL(k_pm_forces, cells_grid(a), dim3(256), 0, st, a, e); }

void lbk_pm_bary(hipStream_t st, const StepArgs &a, const PmExtra &e, const float *f)
{
    hipLaunchKernelGGL(k_pm_bary, cells_grid(a), dim3(256), 0, st, a, e, f);
}

void lbk_pm_feq(hipStream_t st, const StepArgs &a, const PmExtra &e, float *feq)
{
    hipLaunchKernelGGL(k_pm_feq, cells_grid(a), dim3(256), 0, st, a, e, feq);
}

void lbk_pm_collide(hipStream_t st, const StepArgs &a, const PmExtra &e, float *f, const float *feq)
{
    hipLaunchKernelGGL(k_pm_collide, cells_grid(a), dim3(256), 0, st, a, e, f, feq);
}
