// rocket.cpp -- the translation unit of surfactant-propelled colonies: instantiates and launches the kernels of kernels_rocket.h
// (rocket_launch.h).
#include "kernels_rocket.h"

namespace {

dim3 cells_grid(const StepArgs &a) { return dim3((unsigned)((a.nx + 255) / 256), (unsigned)a.ny); }
dim3 step_grid(const StepArgs &a) { return dim3((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + 3) / 4)); }

template <int MODE>
void launch_collide(bool last, hipStream_t st, const RyArgs &m)
{
    if (last) hipLaunchKernelGGL((k_ry_collide<MODE, true>), step_grid(m.a[0]), dim3(64, 4), 0, st, m);
    else hipLaunchKernelGGL((k_ry_collide<MODE, false>), step_grid(m.a[0]), dim3(64, 4), 0, st, m);
}

// RY_ROWS (plan_consts.h) = 10 rows a workgroup: the cell of two lattices with both operands around it takes 134-162 registers, which
// leaves three waves a SIMD, twelve a CU -- one workgroup of 10 + 2 waves fills it and gathers 12 rows for 10
// (tools/kernel_resources.py rocket.cpp k_ry; DESIGN.md section 14 has the table and what 6 and 4 rows measured)
template <int MODE>
void launch_step(bool last, hipStream_t st, const RyArgs &m)
{
    constexpr int R = RY_ROWS;
    const StepArgs &a = m.a[0];
    const dim3 grid((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + R - 1) / R)), block(64, R + 2);
    if (last) hipLaunchKernelGGL((k_ry_step<MODE, R, true>), grid, block, 0, st, m);
    else hipLaunchKernelGGL((k_ry_step<MODE, R, false>), grid, block, 0, st, m);
}

}  // namespace

void lbk_ry_moments(hipStream_t st, const RyArgs &m) { hipLaunchKernelGGL(k_ry_moments, step_grid(m.a[0]), dim3(64, 4), 0, st, m); }

void lbk_ry_collide(int mode, bool last, hipStream_t st, const RyArgs &m)
{
    if (mode == LB_ROCKET_FLOW) launch_collide<LB_ROCKET_FLOW>(last, st, m);
    else launch_collide<LB_ROCKET_FORCES>(last, st, m);
}

void lbk_ry_step(int mode, bool last, hipStream_t st, const RyArgs &m)
{
    if (mode == LB_ROCKET_FLOW) launch_step<LB_ROCKET_FLOW>(last, st, m);
    else launch_step<LB_ROCKET_FORCES>(last, st, m);
}

void lbk_ry_velocity(int mode, hipStream_t st, const RyArgs &m)
{
    if (mode == LB_ROCKET_FLOW) hipLaunchKernelGGL(k_ry_velocity<LB_ROCKET_FLOW>, cells_grid(m.a[0]), dim3(256), 0, st, m);
    else hipLaunchKernelGGL(k_ry_velocity<LB_ROCKET_FORCES>, cells_grid(m.a[0]), dim3(256), 0, st, m);
}

void lbk_ry_forces(int mode, hipStream_t st, const RyArgs &m)
{
    if (mode == LB_ROCKET_FLOW) hipLaunchKernelGGL(k_ry_forces<LB_ROCKET_FLOW>, cells_grid(m.a[0]), dim3(256), 0, st, m);
    else hipLaunchKernelGGL(k_ry_forces<LB_ROCKET_FORCES>, cells_grid(m.a[0]), dim3(256), 0, st, m);
}

void lbk_ry_relax(int mode, hipStream_t st, const RyArgs &m, const float *feq_p, const float *feq_c)
{
    if (mode == LB_ROCKET_FLOW) hipLaunchKernelGGL(k_ry_relax<LB_ROCKET_FLOW>, cells_grid(m.a[0]), dim3(256), 0, st, m, feq_p, feq_c);
    else hipLaunchKernelGGL(k_ry_relax<LB_ROCKET_FORCES>, cells_grid(m.a[0]), dim3(256), 0, st, m, feq_p, feq_c);
}
